// Threshold (range) search and gallery self-join for gfx950 (MI355X).
//
// Replaces the reference's "score everything, keep what clears the threshold" loops
//     similarity = get_similarity(...); keep rows with score >= t       reference code/search_image.py:58-117
//     compare every image with every kept image                          reference tool/find_repeated_in_same_folder.py
// with one primitive: a thresholded MFMA scan that emits CANDIDATE pairs, an exact fp64 recheck of each candidate, and
// a sort.  The [Q,N] score matrix is never written.
//
// Structure ("range search and self-join"):
//   range_scan_kernel          (range_scan_body.h, a template over the element type, E and TRI)
//                              scan_kernel's pipeline (scan_pipeline.h: queries resident as MFMA B fragments, 3-deep LDS
//                              ring filled by global_load_lds, counted waits) with a per-element epilogue: (query, row) is a candidate iff
//                              acc >= threshold - margin(query).  Candidates are compacted per wave and appended to a
//                              workspace list with one 64-bit atomicAdd per wave; the counter keeps counting past the
//                              list's capacity.  TRI: the resident "queries" are gallery rows [b*QMAX, (b+1)*QMAX) and
//                              only rows j > i are scanned (the self-join's upper triangle).
//   range_recheck_kernel       exact fp64 dot (quad_dot, the order oracle/search_ref.c replicates) of every stored
//                              candidate on the ORIGINAL rows; keeps dot64 >= threshold.
//   rocPRIM radix sort         survivors by the key (query << 32) | row, then range_emit_kernel writes the first cap.
// The margin, the wave prefix and the candidate append are shared with the threshold sweep (sweep.hip): range_common.h.
// Why this is exact: margin(q) bounds |acc - dot64| for every row (DESIGN section 3's certificate), so every pair with
// dot64 >= threshold is a candidate, and the recheck decides on dot64 itself.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"
#include "scan_host.h"
#include "radix_sort_host.h"
#include "row_lists.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime.h>

namespace mmr {

// range_scan_kernel, RangeCfg, RangeScanArgs and launch_range_scan: range_scan_body.h; the fp16 kernels are compiled in
// range_f16.hip

// Exact recheck: one candidate per 16-lane group, quad_dot on the original rows (fp32 rows for an fp32 gallery).
// Survivors (key, dot64) are appended with one atomicAdd per wave; counter[1] counts them.
template <typename T, int PER>
__global__ __launch_bounds__(256) void range_recheck_kernel(const T *__restrict__ q, const T *__restrict__ gal, double threshold,
                                                            unsigned long long *__restrict__ counter,
                                                            const uint64_t *__restrict__ cand, int64_t cand_cap,
                                                            uint64_t *__restrict__ surv_k, double *__restrict__ surv_v)
{
    constexpr int E = PER * 64;
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, grp = tid >> 4;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
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
        const bool keep = live && m == 0 && s >= threshold;
        const uint64_t mask = __ballot(keep);
        if (mask) {
            unsigned long long wbase = 0;
            if (lane == 0) wbase = atomicAdd(counter + 1, (unsigned long long)__popcll(mask));
            wbase = __shfl(wbase, 0, 64);
            if (keep) {
                const unsigned long long pos = wbase + __popcll(mask & below);
                surv_k[pos] = key;
                surv_v[pos] = s;
            }
        }
    }
}

__global__ __launch_bounds__(256) void range_emit_kernel(const unsigned long long *__restrict__ counter,
                                                         const uint64_t *__restrict__ sk, const double *__restrict__ sv,
                                                         int64_t cap, float scale, int32_t *__restrict__ out_q,
                                                         int32_t *__restrict__ out_row, float *__restrict__ out_score,
                                                         double *__restrict__ out_dot64, int64_t *__restrict__ counts)
{
    const unsigned long long matches = counter[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = (int64_t)matches;
        counts[1] = (int64_t)counter[0];
    }
    const int64_t n = matches < (unsigned long long)cap ? (int64_t)matches : cap;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t key = sk[i];
        const double d = sv[i];
        out_q[i] = (int32_t)(key >> 32);
        out_row[i] = (int32_t)(key & 0xffffffffu);
        out_score[i] = (float)(d * (double)scale);
        if (out_dot64) out_dot64[i] = d;
    }
}

// fp32 queries -> bf16 (nearest-even) and ||q - bf16(q)||, rounded up: the first tier of the split top-k search does the same
__global__ __launch_bounds__(256) void range_queries_to_bf16_kernel(const float *__restrict__ q, int Q, int E,
                                                                    bf16_t *__restrict__ out, float *__restrict__ qres)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Q) return;
    const float *p = q + (size_t)row * E;
    double ss = 0.0;                                // fp64: the squares of a small query's residuals underflow in fp32
    for (int j = lane; j < E; j += 64) {
        const bf16_t b = f32_to_bf16(p[j]);
        const double d = p[j] - bf16_to_f32(b);     // exact: the residual of a rounding
        ss += d * d;
        out[(size_t)row * E + j] = b;
    }
    ss = wave_sum_f64_butterfly(ss);
    if (lane == 0) qres[row] = norm_upper_f32(ss, 1.00001f);
}

// hi = bf16(gallery) and max_row ||g - hi|| (rounded up) for an fp32 gallery the caller did not split
__global__ __launch_bounds__(256) void range_split_hi_kernel(const float *__restrict__ g, int64_t N, int E, bf16_t *__restrict__ hi,
                                                             unsigned int *__restrict__ out_bits)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < N; r += (int64_t)gridDim.x * 4) {
        const float *p = g + (size_t)r * E;
        double ss = 0.0;
        for (int j = lane; j < E; j += 64) {
            const bf16_t b = f32_to_bf16(p[j]);
            const double d = p[j] - bf16_to_f32(b);
            ss += d * d;
            hi[(size_t)r * E + j] = b;
        }
        ss = wave_sum_f64_butterfly(ss);
        mx = fmax(mx, ss);
    }
    if (lane == 0) atomicMax(out_bits, __float_as_uint(norm_upper_f32(mx, 1.00001f)));
}

int range_queries_to_bf16(const float *q, int Q, int E, bf16_t *out, float *qres, hipStream_t st)
{
    hipLaunchKernelGGL(range_queries_to_bf16_kernel, dim3((Q + 3) / 4), dim3(256), 0, st, q, Q, E, out, qres);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int range_split_hi(const float *g, int64_t N, int E, bf16_t *hi, float *resid, hipStream_t st)
{
    MMR_CHECK_HIP(hipMemsetAsync(resid, 0, sizeof(float), st));
    hipLaunchKernelGGL(range_split_hi_kernel, dim3(grid_1d(N, 4)), dim3(256), 0, st, g, N, E, hi,
                       (unsigned int *)resid);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

struct RangePlan {
    size_t off_cnt, off_nb, off_rb, off_qb, off_qres, off_cand, off_sk, off_sv, off_sk2, off_sv2, off_tmp, off_hi, tmp_bytes, total;
};

static RangePlan make_range_plan(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dt, bool need_hi, bool self_join)
{
    RangePlan p{};
    WsLayout l;
    const int64_t cc = cand_cap > 0 ? cand_cap : 1;
    p.off_cnt = l.take(2 * sizeof(unsigned long long));
    p.off_nb = l.take(sizeof(float));
    p.off_rb = l.take(sizeof(float));
    const bool qsplit = dt == MMR_F32 && !self_join;
    p.off_qb = l.take(qsplit ? (size_t)Q * E * sizeof(bf16_t) : 0);
    p.off_qres = l.take(qsplit ? (size_t)Q * sizeof(float) : 0);
    p.off_cand = l.take((size_t)cc * 8);
    p.off_sk = l.take((size_t)cc * 8);
    p.off_sv = l.take((size_t)cc * 8);
    p.off_sv2 = l.take((size_t)cc * 8);
    p.off_sk2 = p.off_cand;       // sorted keys reuse the candidate list: the recheck is done with it by then
    p.tmp_bytes = sort_bytes<double>(cc);
    p.off_tmp = l.take(p.tmp_bytes > 0 ? p.tmp_bytes : 1);
    p.off_hi = l.take(dt == MMR_F32 && need_hi ? (size_t)N * E * sizeof(bf16_t) : 0);
    p.total = l.off;
    return p;
}

// Shared body of mmr_cosine_range (q != NULL) and mmr_gallery_self_join (q == NULL: the queries are the gallery's rows).
static int range_impl(const char *fn, const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
               int E, double threshold, float scale, float gallery_norm_bound, const float *norm_bound_dev,
               const float *resid_bound_dev, int64_t cap, int64_t cand_cap, int32_t *out_q, int32_t *out_row, float *out_score,
               double *out_dot64, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream,
               const uint32_t *row_mask = nullptr)
{
    const bool tri = q == nullptr;
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.scan_E(E));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(tri || Q >= 1, "%s: Q=%d must be >= 1", fn, Q);
    MMR_CHECK_ARG(threshold == threshold && fabs(threshold) < INFINITY, "%s: threshold must be finite (got %g)", fn, threshold);
    MMR_TRY(ck.scale_finite(scale));
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_CHECK_ARG(cap >= 0 && cand_cap >= 1, "%s: cap=%lld must be >= 0 and cand_cap=%lld >= 1", fn, (long long)cap, (long long)cand_cap);
    MMR_CHECK_ARG(counts != nullptr && workspace != nullptr, "%s: null pointer (counts / workspace)", fn);
    MMR_CHECK_ARG(gallery != nullptr || N == 0, "%s: null pointer (gallery)", fn);
    MMR_CHECK_ARG(cap == 0 || (out_q && out_row && out_score), "%s: null pointer (outputs)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)q | (uintptr_t)gallery | (uintptr_t)gallery_hi, "q / gallery / gallery_hi"));
    MMR_TRY(ck.row_mask(row_mask));
    const int64_t nq = tri ? N : Q;
    const bool split = dtype == MMR_F32;
    const RangePlan p = make_range_plan(N, E, tri ? 0 : Q, cand_cap, dtype, split && gallery_hi == nullptr, tri);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));
    if (p.tmp_bytes == 0) { set_error("%s: sort storage query failed", fn); return MMR_EIO; }

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, 2 * sizeof(unsigned long long), st));
    uint64_t *cand = (uint64_t *)(ws + p.off_cand), *sk = (uint64_t *)(ws + p.off_sk), *sk2 = (uint64_t *)(ws + p.off_sk2);
    double *sv = (double *)(ws + p.off_sv), *sv2 = (double *)(ws + p.off_sv2);

    if (N > 0 && nq > 0) {
        const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, norm_bound_dev, (float *)(ws + p.off_nb), st);
        MMR_TRY(nb.rc);
        ScanOperands ops;       // 16-bit rows: bf16, or fp16 for the <f16_t> scan
        MMR_TRY(scan_operands(split, q, Q, gallery, gallery_hi, resid_bound_dev, N, E, (bf16_t *)(ws + p.off_hi),
                              (float *)(ws + p.off_rb), (bf16_t *)(ws + p.off_qb), (float *)(ws + p.off_qres), st, &ops));
        RangeScanArgs a{};
        a.gal = (const bf16_t *)ops.gal;
        a.N = N;
        a.ntiles = (int)((N + RTILE - 1) / RTILE);
        a.threshold = threshold;
        a.host_bound = nb.host;
        a.dev_bound = nb.dev;
        a.split = split;
        a.resid_dev = ops.resid;
        a.qres = ops.qres;
        a.counter = counter;
        a.cand = cand;
        a.cand_cap = cand_cap;
        a.row_mask = row_mask;
        const int qmax = scan_qmax(E, MMR_BF16);
        if (tri) {
            a.q = a.gal;
            a.nblk = (int)((N + qmax - 1) / qmax);
            a.fblk = RTRI_TPC / (qmax / RTILE);
            a.nchunk = (a.ntiles + RTRI_TPC - 1) / RTRI_TPC;
            // MMR_RANGE_ORDER=block: work items block-major (A/B of the schedule, read per call)
            const char *ord = getenv("MMR_RANGE_ORDER");
            a.order = ord && !strcmp(ord, "block") ? 1 : 0;
            const int64_t F = a.fblk, K = a.nblk / F;
            const int64_t C = a.nchunk;
            const int64_t items = C <= K ? F * C * (C + 1) / 2 : F * K * (K + 1) / 2 + (C - K) * (int64_t)a.nblk;
            MMR_CHECK_ARG(items < 0x7fffffff, "%s: gallery too large for one launch", fn);
            MMR_TRY(dtype == MMR_F16 ? launch_range_scan<f16_t>(E, true, a, (unsigned)items, st)
                                     : launch_range_scan<bf16_t>(E, true, a, (unsigned)items, st));
        } else {
            const ScanTasks t = scan_tasks(a.ntiles);
            a.tpt = t.tpt;
            for (int q0 = 0; q0 < Q; q0 += qmax) {
                a.q0 = q0;
                a.Qc = (Q - q0) < qmax ? (Q - q0) : qmax;
                a.q = (const bf16_t *)ops.q + (size_t)q0 * E;
                MMR_TRY(dtype == MMR_F16 ? launch_range_scan<f16_t>(E, false, a, (unsigned)t.ntasks, st)
                                         : launch_range_scan<bf16_t>(E, false, a, (unsigned)t.ntasks, st));
            }
        }
    }

    ProfScope prof(MMR_PROF_FINALIZE, st);
    const uint64_t pad = (uint64_t)(nq > 0 ? nq : 1) << 32;
    MMR_TRY(fill_u64(sk, cand_cap, pad, st));       // keys above every real key ((query count) << 32) sort last
    if (N > 0 && nq > 0) {
        const dim3 grid(grid_1d(cand_cap, 16, 8192));
        MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
            using T = typename decltype(tag)::type;
            return dispatch_per(E, [&](auto per) -> int {
                hipLaunchKernelGGL((range_recheck_kernel<T, decltype(per)::value>), grid, dim3(256), 0, st,
                                   (const T *)(tri ? gallery : q), (const T *)gallery, threshold, counter, (const uint64_t *)cand,
                                   cand_cap, sk, sv);
                return MMR_OK;
            });
        }));
        MMR_CHECK_LAUNCH();
    }
    // survivors sit in [0, matches) of sk / sv, padding behind them: sort cand_cap keys on the bits that can differ
    MMR_TRY(sort_pairs(fn, ws + p.off_tmp, p.tmp_bytes, sk, sk2, sv, sv2, cand_cap, 0, 32 + bitlen64((uint64_t)(nq > 0 ? nq : 1)), st));
    hipLaunchKernelGGL(range_emit_kernel, dim3(grid_1d(cap)), dim3(256), 0, st,
                       (const unsigned long long *)counter, (const uint64_t *)sk2, (const double *)sv2, cap, scale, out_q,
                       out_row, out_score, out_dot64, counts);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_range_workspace_bytes(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given)
{
    if (N < 0 || Q < 0 || cand_cap < 1 || E < 1 || (dtype != MMR_F32 && dtype != MMR_BF16 && dtype != MMR_F16)) return 0;
    return make_range_plan(N, E, Q, cand_cap, dtype, !gallery_hi_given, false).total;
}

extern "C" int mmr_cosine_range(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                                int E, double threshold, float scale, float gallery_norm_bound,
                                const float *gallery_norm_bound_dev, const float *resid_bound_dev, int64_t cap,
                                int64_t cand_cap, int32_t *out_q, int32_t *out_row, float *out_score, double *out_dot64,
                                int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (q == nullptr) { set_error("mmr_cosine_range: null pointer (q)"); return MMR_EINVAL; }
    return range_impl("mmr_cosine_range", q, gallery, gallery_hi, dtype, Q, N, E, threshold, scale, gallery_norm_bound,
                      gallery_norm_bound_dev, resid_bound_dev, cap, cand_cap, out_q, out_row, out_score, out_dot64, counts,
                      workspace, workspace_bytes, stream);
}

extern "C" int mmr_gallery_self_join(const void *gallery, const void *gallery_hi, mmr_dtype dtype, int64_t N, int E,
                                     double threshold, float scale, float gallery_norm_bound,
                                     const float *gallery_norm_bound_dev, const float *resid_bound_dev, int64_t cap,
                                     int64_t cand_cap, int32_t *out_i, int32_t *out_j, float *out_score, double *out_dot64,
                                     int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    return range_impl("mmr_gallery_self_join", nullptr, gallery, gallery_hi, dtype, 0, N, E, threshold, scale,
                      gallery_norm_bound, gallery_norm_bound_dev, resid_bound_dev, cap, cand_cap, out_i, out_j, out_score,
                      out_dot64, counts, workspace, workspace_bytes, stream);
}

extern "C" int mmr_cosine_range_masked(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q,
                                       int64_t N, int E, double threshold, float scale, float gallery_norm_bound,
                                       const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                       const uint32_t *row_mask, int64_t cap, int64_t cand_cap, int32_t *out_q,
                                       int32_t *out_row, float *out_score, double *out_dot64, int64_t *counts, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (q == nullptr) { set_error("mmr_cosine_range_masked: null pointer (q)"); return MMR_EINVAL; }
    return range_impl("mmr_cosine_range_masked", q, gallery, gallery_hi, dtype, Q, N, E, threshold, scale, gallery_norm_bound,
                      gallery_norm_bound_dev, resid_bound_dev, cap, cand_cap, out_q, out_row, out_score, out_dot64, counts,
                      workspace, workspace_bytes, stream, row_mask);
}

extern "C" int mmr_gallery_self_join_masked(const void *gallery, const void *gallery_hi, mmr_dtype dtype, int64_t N, int E,
                                            double threshold, float scale, float gallery_norm_bound,
                                            const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                            const uint32_t *row_mask, int64_t cap, int64_t cand_cap, int32_t *out_i,
                                            int32_t *out_j, float *out_score, double *out_dot64, int64_t *counts,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    return range_impl("mmr_gallery_self_join_masked", nullptr, gallery, gallery_hi, dtype, 0, N, E, threshold, scale,
                      gallery_norm_bound, gallery_norm_bound_dev, resid_bound_dev, cap, cand_cap, out_i, out_j, out_score,
                      out_dot64, counts, workspace, workspace_bytes, stream, row_mask);
}
