// Exact nearest-centroid assignment of every gallery row for gfx950 (MI355X).
//
// Replaces the Lloyd step of the reference's clustering (KMeans in get_cluster_features / get_text_cluster_features,
// reference code/search_image.py:185-292) for galleries where it is no longer tiny CPU work: labels[r] = the centroid c
// with the largest score(r, c) = dot64(g_r, c) + bias[c], for every row, without an [N, K] score matrix.  A reduction
// over the resident operand for every gallery row, where every other scan reduces over rows per query.
//
// Structure ("Nearest-centroid assignment"):
//   assign_prep_kernel      per centroid: the fp32 bias the scan adds and the margin eps(c) >= |approx - exact score|;
//                           per GROUP of 32 centroids (one wave of a pass) the largest eps, +inf when one is wild.
//   assign_scan_kernel      (assign_scan_body.h, a template over the element type and E) range_scan_kernel's pipeline
//                           with the MFMA operands swapped: a lane holds one tile row against 16 centroids, a wave keeps per row the best approximate score, its centroid and the
//                           runner-up over its 32 centroids and stores the triple, one tile late.
//   assign_merge_kernel     after every pass: folds the pass's groups into a per-row state (winner's lower bound, its
//                           upper bound, the largest upper bound of every other centroid); after the last pass a row
//                           whose winner's lower bound is strictly above every other upper bound is DECIDED, any other
//                           live row is AMBIGUOUS and appended to a row list.
//   assign_recheck_kernel   the ambiguous row's exact fp64 score (quad_dot, the order oracle/search_ref.c replicates)
//                           against all K centroids: largest wins, ties to the lowest c, NaN never wins.
//   assign_score_kernel     optional best64: quad_dot of (row, its centroid) only.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "assign_scan_body.h"
#include "f32_round.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

// assign_scan_kernel, AssignScanArgs and launch_assign_scan: assign_scan_body.h; the fp16 kernels are compiled in
// assign_f16.hip

// One thread per centroid slot i < Kpad (a multiple of 256).  biasf[i] = fp32(bias[i]), -inf for i >= K.
// eps(c) bounds |fl32(acc + biasf) - fl64(dot64 + bias)|: scan_margin's |acc - dot64|, the conversion of the bias
// (2^-24 |bias|, 2^-150 where it is subnormal), the fp32 add (2^-24 (|acc| + |biasf|)) and the fp64 add (2^-53 of the same),
// together below 2^-23 * 1.01 (|bias| + |c| G) + 2^-140.  geps[g] = the largest eps of group g's live centroids, widened
// by 2^-20 for the roundings of the merge's own fp64 arithmetic; +inf when a centroid is wild (scan_margin) or its bias
// would let the fp32 sum overflow: every row is then ambiguous.
template <typename T>
__global__ __launch_bounds__(256) void assign_prep_kernel(const T *__restrict__ cen, int K, int E,
                                                          const double *__restrict__ bias, float host_bound,
                                                          const float *__restrict__ dev_bound, float *__restrict__ biasf,
                                                          double *__restrict__ geps)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < K;
    double qn2 = 0.0;
    if (live) {
        const T *p = cen + (size_t)i * E;
        for (int e = 0; e < E; ++e) { const double x = (double)b16_to_f32<T>(__builtin_bit_cast(uint16_t, p[e])); qn2 += x * x; }
    }
    const double beta = live && bias ? bias[i] : 0.0;
    const ScanMargin mg = scan_margin(qn2, host_bound, dev_bound, 0, nullptr, nullptr, 0);
    float G = host_bound > 0.f ? host_bound : 0.f;
    if (dev_bound) G = fmaxf(G, *dev_bound);
    const double reach = (sqrt(qn2) * 1.0001 * (double)G + fabs(beta)) * 1.01;
    const bool wild = mg.wild || !(reach < (double)__FLT_MAX__);
    double eps = wild ? (double)INFINITY : (mg.eps + 0x1p-23 * reach + 0x1p-140) * (1.0 + 0x1p-20);
    if (!live) eps = 0.0;
    biasf[i] = live ? (float)beta : -INFINITY;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) eps = fmax(eps, __shfl_xor(eps, off, 64));
    if ((threadIdx.x & 31) == 0) geps[i >> 5] = eps;
}

struct AssignMergeArgs {
    const float *best, *second;      // the pass's planes [ng][N]
    const int32_t *arg;
    const double *geps;              // the pass's first group's eps
    int ng;                          // live groups of the pass
    int64_t N;
    int first, last;                 // first / last pass of the call
    float *lo, *own, *rest;          // state [N]: winner's lower bound, its upper bound, max upper bound of the others
    int32_t *win;                    // state [N]: the winner, ASSIGN_OPEN for a row no bound can decide
    const uint32_t *row_mask;
    int32_t *labels;
    unsigned long long *counter;
    int32_t *amb;
    int64_t amb_cap;
};
constexpr int32_t ASSIGN_NONE = -2, ASSIGN_OPEN = -1;

// One thread per row; whole waves run every iteration (the append's prefix is over the wave).
__global__ __launch_bounds__(256) void assign_merge_kernel(AssignMergeArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t N = a.N;
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < N; r0 += (int64_t)gridDim.x * 256) {
        const int64_t r = r0 + threadIdx.x;
        const bool live = r < N && (!a.row_mask || ((a.row_mask[r >> 5] >> (r & 31)) & 1u));
        float L = -INFINITY, H = -INFINITY, U = -INFINITY;
        int32_t I = ASSIGN_NONE;
        if (live) {
            if (!a.first) { L = a.lo[r]; H = a.own[r]; U = a.rest[r]; I = a.win[r]; }
            for (int g = 0; g < a.ng; ++g) {
                const size_t at = (size_t)g * (size_t)N + (size_t)r;
                const float b = a.best[at], s = a.second[at];
                const int32_t c = a.arg[at];
                const double eps = a.geps[g];
                if (c < 0 || !(eps < (double)INFINITY) || I == ASSIGN_OPEN) { I = ASSIGN_OPEN; continue; }
                const float lo = f32_down((double)b - eps), hi1 = f32_up((double)b + eps), hi2 = f32_up((double)s + eps);
                if (I == ASSIGN_NONE || lo > L) {
                    U = fmaxf(U, fmaxf(H, hi2));          // the old winner and the new group's other centroids
                    L = lo; H = hi1; I = c;
                } else {
                    U = fmaxf(U, hi1);
                }
            }
            if (!a.last) { a.lo[r] = L; a.own[r] = H; a.rest[r] = U; a.win[r] = I; }
        }
        if (a.last) {
            const bool decided = live && I >= 0 && L > U;
            if (r < N) a.labels[r] = decided ? I : -1;
            const bool open = live && !decided;
            const WavePrefix wp = wave_prefix(open ? 1 : 0, lane);
            if (wp.total > 0) {
                unsigned long long wbase = 0;
                if (lane == 0) wbase = atomicAdd(a.counter, (unsigned long long)wp.total);
                wbase = __shfl(wbase, 0, 64);
                const unsigned long long pos = wbase + (unsigned long long)wp.before;
                if (open && pos < (unsigned long long)a.amb_cap) a.amb[pos] = (int32_t)r;
            }
        }
    }
}

// Exact recheck: one ambiguous row per 16-lane group, quad_dot against every centroid in ascending c.  The strict
// comparison keeps the lowest c among equal scores; a NaN score never replaces anything.
template <typename T, int PER>
__global__ __launch_bounds__(256) void assign_recheck_kernel(const T *__restrict__ gal, const T *__restrict__ cen, int K,
                                                             const double *__restrict__ bias,
                                                             const unsigned long long *__restrict__ counter,
                                                             const int32_t *__restrict__ amb, int64_t amb_cap,
                                                             int32_t *__restrict__ labels, int64_t *__restrict__ counts)
{
    constexpr int E = PER * 64;
    const int tid = threadIdx.x, m = tid & 15, grp = tid >> 4;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)amb_cap ? (int64_t)nc : amb_cap;
    if (blockIdx.x == 0 && tid == 0) {
        counts[0] = n;
        counts[1] = (int64_t)nc;
    }
    for (int64_t b0 = (int64_t)blockIdx.x * 16; b0 < n; b0 += (int64_t)gridDim.x * 16) {
        const int64_t i = b0 + grp;
        const bool live = i < n;
        const int64_t row = amb[live ? i : b0];
        QuadQuery<T, PER> gr;
        gr.load(gal + (size_t)row * E, m);
        double best = 0.0;
        int32_t lab = -1;
        for (int c = 0; c < K; ++c) {
            QuadRow<T, PER> cr;
            cr.load(cen + (size_t)c * E, m);
            double s = quad_dot<T, PER>(gr, cr);
            if (bias) s += bias[c];
            if (s == s && (lab < 0 || s > best)) { best = s; lab = c; }
        }
        if (live && m == 0) labels[row] = lab;
    }
}

// best64[r] = the exact score of (r, labels[r]), NaN where the label is -1: one row per 16-lane group
template <typename T, int PER>
__global__ __launch_bounds__(256) void assign_score_kernel(const T *__restrict__ gal, const T *__restrict__ cen,
                                                           const double *__restrict__ bias, const int32_t *__restrict__ labels,
                                                           int64_t N, double *__restrict__ best64)
{
    constexpr int E = PER * 64;
    const int tid = threadIdx.x, m = tid & 15, grp = tid >> 4;
    for (int64_t b0 = (int64_t)blockIdx.x * 16; b0 < N; b0 += (int64_t)gridDim.x * 16) {
        const int64_t i = b0 + grp;
        const bool live = i < N;
        const int64_t row = live ? i : b0;
        const int32_t lab = labels[row];
        QuadQuery<T, PER> gr;
        gr.load(gal + (size_t)row * E, m);
        QuadRow<T, PER> cr;
        cr.load(cen + (size_t)(lab < 0 ? 0 : lab) * E, m);
        double s = quad_dot<T, PER>(gr, cr);
        if (bias) s += bias[lab < 0 ? 0 : lab];
        if (live && m == 0) best64[row] = lab < 0 ? (double)NAN : s;
    }
}

struct AssignPlan {
    int kpad, waves;
    size_t off_cnt, off_nb, off_biasf, off_geps, off_best, off_second, off_arg, off_lo, off_own, off_rest, off_win, off_amb, total;
};

static AssignPlan make_assign_plan(int64_t N, int E, int K, int64_t amb_cap)
{
    AssignPlan p{};
    p.kpad = (int)align_up((size_t)K, 256);
    p.waves = scan_qmax(E, MMR_BF16) / AGROUP;
    const size_t plane = (size_t)p.waves * (size_t)N * 4, rows = (size_t)N * 4;
    WsLayout l;
    p.off_cnt = l.take(sizeof(unsigned long long));
    p.off_nb = l.take(sizeof(float));
    p.off_biasf = l.take((size_t)p.kpad * 4);
    p.off_geps = l.take((size_t)(p.kpad / AGROUP) * 8);
    p.off_best = l.take(plane);
    p.off_second = l.take(plane);
    p.off_arg = l.take(plane);
    p.off_lo = l.take(rows);
    p.off_own = l.take(rows);
    p.off_rest = l.take(rows);
    p.off_win = l.take(rows);
    p.off_amb = l.take((size_t)(amb_cap > 0 ? amb_cap : 1) * 4);
    p.total = l.off;
    return p;
}

constexpr int ASSIGN_K_MAX = 1 << 24;

}  // namespace mmr

using namespace mmr;

static bool assign_sizes_ok(int64_t N, int E, int K, int64_t amb_cap, mmr_dtype dtype)
{
    return N >= 0 && N < 0x7fffffff && K >= 1 && K <= ASSIGN_K_MAX && amb_cap >= 1 && scan_supports_E(E) &&
           (dtype == MMR_BF16 || dtype == MMR_F16);
}

extern "C" size_t mmr_assign_workspace_bytes(int64_t N, int E, int K, int64_t amb_cap, mmr_dtype dtype)
{
    if (!assign_sizes_ok(N, E, K, amb_cap, dtype)) return 0;
    return make_assign_plan(N, E, K, amb_cap).total;
}

extern "C" int mmr_cosine_assign(const void *gallery, const void *centroids, mmr_dtype dtype, int64_t N, int K, int E,
                                 const double *bias_dev, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                                 const uint32_t *row_mask, int64_t amb_cap, int32_t *labels, double *best64, int64_t *counts,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_cosine_assign";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    if (dtype == MMR_F32) {
        set_error("%s: fp32 galleries are not supported (bf16 or fp16 only: the 16-bit scan of an fp32 gallery leaves too many rows undecided)", fn);
        return MMR_ENOTSUP;
    }
    MMR_TRY(ck.scan_E(E));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(K >= 1 && K <= ASSIGN_K_MAX, "%s: K=%d outside [1, 2^24]", fn, K);
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_CHECK_ARG(amb_cap >= 1, "%s: amb_cap=%lld must be >= 1", fn, (long long)amb_cap);
    MMR_CHECK_ARG(centroids != nullptr, "%s: null pointer (centroids)", fn);
    MMR_CHECK_ARG(counts != nullptr && workspace != nullptr, "%s: null pointer (counts / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr) || N == 0, "%s: null pointer (gallery / labels)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)centroids | (uintptr_t)gallery, "centroids / gallery"));
    MMR_CHECK_ARG((((uintptr_t)bias_dev | (uintptr_t)best64 | (uintptr_t)counts) & 7) == 0, "%s: bias_dev / best64 / counts must be 8-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)labels & 3) == 0, "%s: labels must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    MMR_TRY(ck.row_mask(row_mask));
    const AssignPlan p = make_assign_plan(N, E, K, amb_cap);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {       // no rows: no labels; only the counts are written
        MMR_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
        return MMR_OK;
    }
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
    float *biasf = (float *)(ws + p.off_biasf);
    double *geps = (double *)(ws + p.off_geps);

    const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, gallery_norm_bound_dev, (float *)(ws + p.off_nb), st);
    MMR_TRY(nb.rc);
    {
        ProfScope prof(MMR_PROF_ROWWISE, st);
        if (dtype == MMR_F16)
            hipLaunchKernelGGL(assign_prep_kernel<f16_t>, dim3(p.kpad / 256), dim3(256), 0, st, (const f16_t *)centroids, K, E, bias_dev,
                               nb.host, nb.dev, biasf, geps);
        else
            hipLaunchKernelGGL(assign_prep_kernel<bf16_t>, dim3(p.kpad / 256), dim3(256), 0, st, (const bf16_t *)centroids, K, E, bias_dev,
                               nb.host, nb.dev, biasf, geps);
        MMR_CHECK_LAUNCH();
    }

    AssignScanArgs a{};
    a.gal = (const bf16_t *)gallery;
    a.N = N;
    a.ntiles = (int)((N + RTILE - 1) / RTILE);
    a.biasf = biasf;
    a.row_mask = row_mask;
    a.best = (float *)(ws + p.off_best);
    a.second = (float *)(ws + p.off_second);
    a.arg = (int32_t *)(ws + p.off_arg);
    AssignMergeArgs m{};
    m.best = a.best; m.second = a.second; m.arg = a.arg;
    m.N = N;
    m.lo = (float *)(ws + p.off_lo); m.own = (float *)(ws + p.off_own); m.rest = (float *)(ws + p.off_rest);
    m.win = (int32_t *)(ws + p.off_win);
    m.row_mask = row_mask;
    m.labels = labels;
    m.counter = counter;
    m.amb = (int32_t *)(ws + p.off_amb);
    m.amb_cap = amb_cap;
    const int qmax = p.waves * AGROUP;
    const ScanTasks t = scan_tasks(a.ntiles);
    a.tpt = t.tpt;
    for (int c0 = 0; c0 < K; c0 += qmax) {
        a.c0 = c0;
        a.Kc = (K - c0) < qmax ? (K - c0) : qmax;
        a.cen = (const bf16_t *)centroids + (size_t)c0 * E;
        MMR_TRY(dtype == MMR_F16 ? launch_assign_scan<f16_t>(E, a, (unsigned)t.ntasks, st) : launch_assign_scan<bf16_t>(E, a, (unsigned)t.ntasks, st));
        m.geps = geps + c0 / AGROUP;
        m.ng = (a.Kc + AGROUP - 1) / AGROUP;
        m.first = c0 == 0;
        m.last = c0 + qmax >= K;
        ProfScope prof(MMR_PROF_FINALIZE, st);
        hipLaunchKernelGGL(assign_merge_kernel, dim3(grid_1d(N)), dim3(256), 0, st, m);
        MMR_CHECK_LAUNCH();
    }

    ProfScope prof(MMR_PROF_FINALIZE, st);
    const dim3 grid(grid_1d(amb_cap, 16, 8192));
    MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        if constexpr (__is_same(T, float)) {
            return MMR_ENOTSUP;       // refused above
        } else {
            return dispatch_per(E, [&](auto per) -> int {
                hipLaunchKernelGGL((assign_recheck_kernel<T, decltype(per)::value>), grid, dim3(256), 0, st, (const T *)gallery,
                                   (const T *)centroids, K, bias_dev, (const unsigned long long *)counter, (const int32_t *)m.amb,
                                   amb_cap, labels, counts);
                if (best64)
                    hipLaunchKernelGGL((assign_score_kernel<T, decltype(per)::value>), dim3(grid_1d(N, 16, 8192)), dim3(256), 0, st,
                                       (const T *)gallery, (const T *)centroids, bias_dev, (const int32_t *)labels, N, best64);
                return MMR_OK;
            });
        }
    }));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
