// Labelled threshold sweep for gfx950 (MI355X): exact TP / FP counts at every point of a threshold grid, one pass.
//
// Replaces the tail every retrieval driver of the reference shares -- score the gallery against a few class vectors,
// split the scores by label, count `pos >= t` and `neg >= t` over a grid --
//     eval_threshold / find_thresholds      reference code/search_image.py:39-103, code/main_custom.py:27-92
//     evaluate_thresholds                   reference CLIP/lab3.py:39-65, CLIP/union_dataset.py:46-61
// without the [Q,N] score matrix and without one range search per grid point.
//
// Structure ("Threshold sweep"):
//   sweep_scan_kernel              (sweep_scan_body.h) range_scan_kernel's pipeline (scan_pipeline.h: queries resident as MFMA B fragments,
//                                  LDS ring filled by global_load_lds, counted waits) with a binning epilogue.  With
//                                  a = the approximate dot and eps = margin(query) (range_common.h), a pair is
//                                    DECIDED    when no threshold lies in [a - eps, a + eps]: the exact dot has a's bin,
//                                               bin = #{i : thresholds[i] <= a}; one LDS atomic on the workgroup's
//                                               histogram word (query, bin): negatives in the low half, positives in
//                                               the high half;
//                                    AMBIGUOUS  otherwise (or a is not finite, or the query is wild): a candidate,
//                                               (query << 32) | row, as in range_scan_kernel.  A grid makes candidates
//                                               common (the share of pairs within eps of a grid point), and a
//                                               returning global atomic inside the ring drains its prefetch, so each
//                                               wave stages its candidates in LDS and appends them in batches: one
//                                               64-bit atomicAdd per batch, the counter runs past the capacity.
//                                  When the task ends the non-zero words go to the global int64 histogram.
//   sweep_recheck_kernel           exact fp64 dot (quad_dot on the ORIGINAL rows) of every stored candidate, NaN dropped,
//                                  bin by binary search over the fp64 grid, one global atomic.
//   sweep_finish_kernel            hist[Q,2,T+1] -> ge (suffix sums), total (row sums), counts.
// Integer atomics only: the result does not depend on arrival order.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "sweep_scan_body.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

// sweep_scan_kernel, SweepCfg, SweepScanArgs, the staging constants and launch_sweep_scan: sweep_scan_body.h; the fp16
// kernels are compiled in sweep_f16.hip, the per-query ones in sweep_qmask.hip

// LDS left for the counts and the candidate staging
static int sweep_lds_room(int E, int T)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        return SWEEP_LDS_MAX - C::RING - SWEEP_LABEL_BYTES - sweep_grid_bytes(T);
    });
}
static int sweep_hist_bytes(int rows, int T) { return (rows * (T + 1) * 4 + 7) / 8 * 8; }      // the staging behind it is 8-byte aligned
static int sweep_waves(int E) { return E <= 512 ? 8 : 4; }
// per-query margin / target / flags (16 B) of the multiplying waves, the counts, every wave's staging
static int sweep_lds_need(int E, int rows, int T, int stage)
{
    return (rows + 31) / 32 * 32 * 16 + sweep_hist_bytes(rows, T) + sweep_waves(E) * stage * 8;
}

// queries per gallery pass: what fits in LDS beside the ring, the labels and the grid (their counts plus the least
// staging for each wave that multiplies), at most the kernel's QMAX
// qm_tpt > 0 (mmr_threshold_sweep_qmasked): tiles per task; the task's mask words, [tile][rows + 1], take their share
static int sweep_qmask_bytes(int rows, int qm_tpt) { return qm_tpt * (rows + 1) * 4; }
static int sweep_queries_per_pass(int E, int T, int qm_tpt = 0)
{
    const int room = sweep_lds_room(E, T);
    int rows = scan_dispatch_E(E, [&](auto e) { return (int)SweepCfg<decltype(e)::value>::QCAP; });
    while (rows > 1 && sweep_lds_need(E, rows, T, SWEEP_STAGE_MIN) + sweep_qmask_bytes(rows, qm_tpt) > room) --rows;
    return rows;
}
// staging entries per wave when a pass holds `rows` queries: the LDS that is left, at most SWEEP_STAGE_MAX
static int sweep_stage_entries(int E, int T, int rows, int qm_tpt = 0)
{
    const int left = (sweep_lds_room(E, T) - sweep_lds_need(E, rows, T, 0) - sweep_qmask_bytes(rows, qm_tpt)) / sweep_waves(E) / 8;
    return left < SWEEP_STAGE_MAX ? left : SWEEP_STAGE_MAX;
}


// The fp32 images of the grid the scan compares against, with sentinels: down[0] = up[0] = -inf,
// down[k] = thresholds[k-1] rounded down, up[k] = thresholds[k-1] rounded up, down[T+1] = up[T+1] = +inf.
// The grid arrives by value, SWEEP_CHUNK points per launch: the caller's host array is read before the call returns.
constexpr int SWEEP_CHUNK = 256;
struct SweepGridChunk {
    double t[SWEEP_CHUNK];
};
__global__ __launch_bounds__(SWEEP_CHUNK) void sweep_grid_kernel(SweepGridChunk ch, int off, int n, int T, double *__restrict__ thr64,
                                                                float *__restrict__ grid32)
{
    const int i = threadIdx.x;
    float *down = grid32, *up = grid32 + (T + 2);
    if (i < n) {
        const double t = ch.t[i];
        thr64[off + i] = t;
        down[off + i + 1] = f32_down(t);
        up[off + i + 1] = f32_up(t);
    }
    if (off == 0 && i == 0) {
        down[0] = -INFINITY; up[0] = -INFINITY;
        down[T + 1] = INFINITY; up[T + 1] = INFINITY;
    }
}

// Exact recheck: one candidate per 16-lane group, quad_dot on the original rows (fp32 rows for an fp32 gallery).
// The fp64 grid sits in LDS (at most 8 KiB): the bin search is ten dependent reads per candidate.
template <typename T, int PER>
__global__ __launch_bounds__(256) void sweep_recheck_kernel(const T *__restrict__ q, const T *__restrict__ gal,
                                                            const int32_t *__restrict__ labels, const int32_t *__restrict__ targets,
                                                            const double *__restrict__ thr64, int nthr,
                                                            const unsigned long long *__restrict__ counter,
                                                            const uint64_t *__restrict__ cand, int64_t cand_cap,
                                                            unsigned long long *__restrict__ hist)
{
    constexpr int E = PER * 64;
    extern __shared__ double sthr[];
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, grp = tid >> 4;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
    if ((int64_t)blockIdx.x * 16 >= n) return;
    for (int i = tid; i < nthr; i += 256) sthr[i] = thr64[i];
    __syncthreads();
    for (int64_t b0 = (int64_t)blockIdx.x * 16; b0 < n; b0 += (int64_t)gridDim.x * 16) {
        const int64_t i = b0 + grp;
        const bool live = i < n;
        const uint64_t key = cand[live ? i : b0];
        const int64_t qi = (int64_t)(key >> 32), row = (int64_t)(key & 0xffffffffu);
        QuadQuery<T, PER> qq;
        qq.load(q + (size_t)qi * E, m);
        QuadRow<T, PER> gr;
        gr.load(gal + (size_t)row * E, m);
        const double s = quad_dot<T, PER>(qq, gr);
        if (live && m == 0 && s == s) {
            int l = 0, u = nthr;                     // bin = #{k : thresholds[k] <= s}
            while (l < u) {
                const int mid = (l + u) >> 1;
                if (sthr[mid] <= s) l = mid + 1; else u = mid;
            }
            const int cls = labels[row] == targets[qi] ? 1 : 0;
            atomicAdd(hist + ((size_t)qi * 2 + cls) * (nthr + 1) + l, 1ull);
        }
    }
}

// One workgroup per (query, class): ge[i] = rows in the bins above i (suffix sums), total = all bins
constexpr int SWEEP_FIN_PER = (MMR_SWEEP_T_MAX + 1 + 255) / 256;
__global__ __launch_bounds__(256) void sweep_finish_kernel(const unsigned long long *__restrict__ hist, int T,
                                                           const unsigned long long *__restrict__ counter, int64_t cand_cap,
                                                           int64_t *__restrict__ ge, int64_t *__restrict__ total,
                                                           int64_t *__restrict__ counts)
{
    __shared__ long long part[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r == 0 && tid == 0) {
        const unsigned long long nc = counter[0];
        counts[0] = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
        counts[1] = (int64_t)nc;
    }
    const unsigned long long *h = hist + (size_t)r * (T + 1);
    const int b0 = tid * SWEEP_FIN_PER;
    long long v[SWEEP_FIN_PER], s = 0;
#pragma unroll
    for (int j = 0; j < SWEEP_FIN_PER; ++j) {
        v[j] = b0 + j <= T ? (long long)h[b0 + j] : 0;
        s += v[j];
    }
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // inclusive suffix scan over the threads
        const long long add = tid + off < 256 ? part[tid + off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    long long run = part[tid] - s;                      // the bins of the threads above
#pragma unroll
    for (int j = SWEEP_FIN_PER - 1; j >= 0; --j) {
        const int b = b0 + j;
        run += v[j];
        if (b >= 1 && b <= T) ge[(size_t)r * T + b - 1] = run;
        if (b == 0) total[r] = run;
    }
}

struct SweepPlan {
    size_t off_cnt, off_nb, off_rb, off_qb, off_qres, off_thr, off_grid, off_hist, off_cand, off_hi, hist_bytes, total;
};

static SweepPlan make_sweep_plan(int64_t N, int E, int Q, int T, int64_t cand_cap, mmr_dtype dt, bool need_hi)
{
    SweepPlan p{};
    WsLayout l;
    const int64_t cc = cand_cap > 0 ? cand_cap : 1;
    p.off_cnt = l.take(2 * sizeof(unsigned long long));
    p.off_nb = l.take(sizeof(float));
    p.off_rb = l.take(sizeof(float));
    const bool qsplit = dt == MMR_F32;
    p.off_qb = l.take(qsplit ? (size_t)Q * E * sizeof(bf16_t) : 0);
    p.off_qres = l.take(qsplit ? (size_t)Q * sizeof(float) : 0);
    p.off_thr = l.take((size_t)T * sizeof(double));
    p.off_grid = l.take((size_t)sweep_grid_bytes(T));
    p.hist_bytes = (size_t)Q * 2 * (T + 1) * sizeof(unsigned long long);
    p.off_hist = l.take(p.hist_bytes);
    p.off_cand = l.take((size_t)cc * 8);
    p.off_hi = l.take(dt == MMR_F32 && need_hi ? (size_t)N * E * sizeof(bf16_t) : 0);
    p.total = l.off;
    return p;
}

// The LDS plan of one pass and its launch.  f16: a.q / a.gal point at fp16 elements.  qm (nullable): the per-query masks
// of this pass.
static int launch_sweep_pass(int E, const SweepScanArgs &a, unsigned grid, hipStream_t st, bool f16, const QMaskArgs *qm = nullptr)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        static_assert(C::WAVES == (decltype(e)::value <= 512 ? 8 : 4), "sweep_waves");
        const int lds = C::RING + SWEEP_LABEL_BYTES + sweep_grid_bytes(a.T) + sweep_lds_need(decltype(e)::value, a.hrows, a.T, a.stage) +
                        (qm ? sweep_qmask_bytes(a.hrows, a.tpt) : 0);
        if (lds > SWEEP_LDS_MAX) { set_error("mmr_threshold_sweep: LDS plan %d > %d", lds, SWEEP_LDS_MAX); return (int)MMR_EIO; }
        if (qm) return launch_sweep_scan_qmasked(E, f16, a, *qm, grid, lds, st);
        return f16 ? launch_sweep_scan<f16_t>(E, a, grid, lds, st) : launch_sweep_scan<bf16_t>(E, a, grid, lds, st);
    });
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_sweep_workspace_bytes(int64_t N, int E, int Q, int T, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given)
{
    if (N < 0 || Q < 0 || T < 1 || T > MMR_SWEEP_T_MAX || cand_cap < 1 || E < 1 || (dtype != MMR_F32 && dtype != MMR_BF16 && dtype != MMR_F16)) return 0;
    return make_sweep_plan(N, E, Q, T, cand_cap, dtype, !gallery_hi_given).total;
}

// mmr_threshold_sweep (qmasked = false: row_masks / mask_stride unused) and mmr_threshold_sweep_qmasked
static int sweep_impl(const char *fn, bool qmasked, const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype,
                      int Q, int64_t N, int E, const int32_t *labels, const int32_t *targets, const double *thresholds_host, int T,
                      float gallery_norm_bound, const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                      const uint32_t *row_masks, int64_t mask_stride, const uint32_t *row_mask, int64_t cand_cap, int64_t *ge,
                      int64_t *total, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.scan_E(E));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(Q >= 1, "%s: Q=%d must be >= 1", fn, Q);
    MMR_CHECK_ARG(T >= 1 && T <= MMR_SWEEP_T_MAX, "%s: T=%d outside [1, %d]", fn, T, MMR_SWEEP_T_MAX);
    MMR_CHECK_ARG(thresholds_host != nullptr, "%s: null pointer (thresholds_host)", fn);
    for (int i = 0; i < T; ++i) {
        const double t = thresholds_host[i];
        MMR_CHECK_ARG(t == t && fabs(t) < INFINITY, "%s: thresholds[%d] must be finite (got %g)", fn, i, t);
        MMR_CHECK_ARG(i == 0 || thresholds_host[i - 1] < t, "%s: thresholds must be strictly ascending (thresholds[%d] = %g after %g)",
                      fn, i, t, i ? thresholds_host[i - 1] : 0.0);
    }
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_CHECK_ARG(cand_cap >= 1, "%s: cand_cap=%lld must be >= 1", fn, (long long)cand_cap);
    MMR_CHECK_ARG(q != nullptr && targets != nullptr, "%s: null pointer (q / targets)", fn);
    MMR_CHECK_ARG(ge != nullptr && total != nullptr && counts != nullptr && workspace != nullptr,
                  "%s: null pointer (ge / total / counts / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr) || N == 0, "%s: null pointer (gallery / labels)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)q | (uintptr_t)gallery | (uintptr_t)gallery_hi, "q / gallery / gallery_hi"));
    MMR_CHECK_ARG((((uintptr_t)labels | (uintptr_t)targets) & 3) == 0, "%s: labels / targets must be 4-byte aligned", fn);
    MMR_TRY(ck.row_mask(row_mask));
    if (qmasked) {
        MMR_CHECK_ARG(row_masks != nullptr || N == 0, "%s: null pointer (row_masks)", fn);
        MMR_CHECK_ARG(((uintptr_t)row_masks & 3) == 0, "%s: row_masks must be 4-byte aligned", fn);
        MMR_CHECK_ARG(mask_stride >= (N + 31) / 32, "%s: mask_stride=%lld below ceil(N/32)=%lld words", fn, (long long)mask_stride,
                      (long long)((N + 31) / 32));
    }
    const bool split = dtype == MMR_F32;
    const SweepPlan p = make_sweep_plan(N, E, Q, T, cand_cap, dtype, split && gallery_hi == nullptr);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    unsigned long long *hist = (unsigned long long *)(ws + p.off_hist);
    double *thr64 = (double *)(ws + p.off_thr);
    float *grid32 = (float *)(ws + p.off_grid);
    uint64_t *cand = (uint64_t *)(ws + p.off_cand);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, 2 * sizeof(unsigned long long), st));
    MMR_CHECK_HIP(hipMemsetAsync(hist, 0, p.hist_bytes, st));
    for (int off = 0; off < T; off += SWEEP_CHUNK) {
        SweepGridChunk ch;
        const int n = T - off < SWEEP_CHUNK ? T - off : SWEEP_CHUNK;
        for (int i = 0; i < SWEEP_CHUNK; ++i) ch.t[i] = i < n ? thresholds_host[off + i] : 0.0;
        hipLaunchKernelGGL(sweep_grid_kernel, dim3(1), dim3(SWEEP_CHUNK), 0, st, ch, off, n, T, thr64, grid32);
        MMR_CHECK_LAUNCH();
    }

    if (N > 0) {
        const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, gallery_norm_bound_dev, (float *)(ws + p.off_nb), st);
        MMR_TRY(nb.rc);
        ScanOperands ops;       // 16-bit rows: bf16, or fp16 for the <f16_t> scan
        MMR_TRY(scan_operands(split, q, Q, gallery, gallery_hi, resid_bound_dev, N, E, (bf16_t *)(ws + p.off_hi),
                              (float *)(ws + p.off_rb), (bf16_t *)(ws + p.off_qb), (float *)(ws + p.off_qres), st, &ops));
        SweepScanArgs a{};
        a.gal = (const bf16_t *)ops.gal;
        a.resid_dev = ops.resid;
        a.qres = ops.qres;
        a.N = N;
        a.ntiles = (int)((N + RTILE - 1) / RTILE);
        a.host_bound = nb.host;
        a.dev_bound = nb.dev;
        a.split = split;
        a.counter = counter;
        a.cand = cand;
        a.cand_cap = cand_cap;
        a.row_mask = qmasked ? nullptr : row_mask;       // the per-query scan takes the shared mask in QMaskArgs
        a.labels = labels;
        a.targets = targets;
        a.grid32 = grid32;
        a.T = T;
        a.hist = hist;
        a.gt0 = (float)thresholds_host[0];
        const double span = thresholds_host[T - 1] - thresholds_host[0];
        a.ginv = T > 1 ? (float)((double)(T - 1) / span) : 0.f;
        if (!(a.ginv < INFINITY) || !(fabsf(a.gt0) < INFINITY)) { a.ginv = 0.f; a.gt0 = 0.f; }   // the guess is only a guess
        const ScanTasks t = scan_tasks(a.ntiles);
        a.tpt = t.tpt;
        const int qm_tpt = qmasked ? t.tpt : 0;
        const int qpp = sweep_queries_per_pass(E, T, qm_tpt);
        a.hrows = Q < qpp ? Q : qpp;
        a.stage = sweep_stage_entries(E, T, a.hrows, qm_tpt);
        for (int q0 = 0; q0 < Q; q0 += qpp) {
            a.q0 = q0;
            a.Qc = (Q - q0) < qpp ? (Q - q0) : qpp;
            a.ncw = (a.Qc + 31) / 32;
            a.q = (const bf16_t *)ops.q + (size_t)q0 * E;
            const QMaskArgs qm{qmasked ? row_masks + (size_t)q0 * mask_stride : nullptr, mask_stride, row_mask};
            MMR_TRY(launch_sweep_pass(E, a, (unsigned)t.ntasks, st, dtype == MMR_F16, qmasked ? &qm : nullptr));
        }
        ProfScope prof(MMR_PROF_FINALIZE, st);
        const dim3 grid(grid_1d(cand_cap, 16, 8192));
        MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
            using ET = typename decltype(tag)::type;
            return dispatch_per(E, [&](auto per) -> int {
                hipLaunchKernelGGL((sweep_recheck_kernel<ET, decltype(per)::value>), grid, dim3(256), T * sizeof(double), st,
                                   (const ET *)q, (const ET *)gallery, labels, targets, (const double *)thr64, T,
                                   (const unsigned long long *)counter, (const uint64_t *)cand, cand_cap, hist);
                return MMR_OK;
            });
        }));
        MMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sweep_finish_kernel, dim3((unsigned)(2 * Q)), dim3(256), 0, st, (const unsigned long long *)hist, T,
                       (const unsigned long long *)counter, cand_cap, ge, total, counts);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_threshold_sweep(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                                   int E, const int32_t *labels, const int32_t *targets, const double *thresholds_host, int T,
                                   float gallery_norm_bound, const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                   const uint32_t *row_mask, int64_t cand_cap, int64_t *ge, int64_t *total, int64_t *counts,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    return sweep_impl("mmr_threshold_sweep", false, q, gallery, gallery_hi, dtype, Q, N, E, labels, targets, thresholds_host, T,
                      gallery_norm_bound, gallery_norm_bound_dev, resid_bound_dev, nullptr, 0, row_mask, cand_cap, ge, total, counts,
                      workspace, workspace_bytes, stream);
}

extern "C" int mmr_threshold_sweep_qmasked(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q,
                                           int64_t N, int E, const int32_t *labels, const int32_t *targets,
                                           const double *thresholds_host, int T, float gallery_norm_bound,
                                           const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                           const uint32_t *row_masks, int64_t mask_stride, const uint32_t *row_mask,
                                           int64_t cand_cap, int64_t *ge, int64_t *total, int64_t *counts, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return sweep_impl("mmr_threshold_sweep_qmasked", true, q, gallery, gallery_hi, dtype, Q, N, E, labels, targets, thresholds_host,
                      T, gallery_norm_bound, gallery_norm_bound_dev, resid_bound_dev, row_masks, mask_stride, row_mask, cand_cap, ge,
                      total, counts, workspace, workspace_bytes, stream);
}
