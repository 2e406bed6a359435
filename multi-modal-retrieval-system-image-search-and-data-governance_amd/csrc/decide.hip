// Per-query threshold decisions as packed row masks for gfx950 (MI355X).
//
// Replaces the tail of the reference's prediction pipelines
//     (similarity < threshold).int() per class row                     reference code/merge_dataset.py:259-311
//     preds = [0 if (cn == 0 or en == 0) else 1 ...]                    reference code/merge_dataset.py:440
//     the union's TP / FP / FN per class                                reference CLIP/union_dataset.py:64-231
// with one primitive: Q queries with Q thresholds of their own, one pass over the gallery, Q exact row masks in the
// word format of mmr_row_mask_pack.  No pair list, no sort: the answer is Q * ceil(N/32) words whatever share passes.
//
// Structure ("decision masks"):
//   decide_scan_kernel      (decide_scan_body.h, a template over the element type and E) range_scan_kernel's non-TRI
//                           pipeline (scan_pipeline.h) with a deciding epilogue: per lane two fp32 thresholds, thr +- margin(query) rounded outward; acc >= thr_hi sets the pair's bit,
//                           acc < thr_lo leaves it clear, anything else is a CANDIDATE (bit clear, pair appended as in
//                           range search).  A 32-row tile is one word per query: the two half-lanes of a query combine
//                           their 16 bits with one shuffle and one lane stores the word, one tile late.
//   decide_recheck_kernel   exact fp64 dot (quad_dot, the order oracle/search_ref.c replicates) of every stored
//                           candidate on the ORIGINAL rows; dot64 >= threshold ORs the bit in.  OR is order-free.
//   row_mask_combine_kernel / decision_counts_kernel   word-wise OR / AND / AND-NOT, and TP / FP / POS / NEG of masks.
// Why this is exact: margin(q) bounds |acc - dot64| for every row (DESIGN section 3's certificate), so a pair the scan
// decides is decided as dot64 would, and the recheck decides the rest on dot64 itself.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "decide_scan_body.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

// decide_scan_kernel, DecideScanArgs and launch_decide_scan: decide_scan_body.h; the fp16 kernels are compiled in
// decide_f16.hip

// Exact recheck: one candidate per 16-lane group, quad_dot on the original rows (fp32 rows for an fp32 gallery).  A
// candidate's row is live (the scan appends no other), so the bit depends on the dot alone.
template <typename T, int PER>
__global__ __launch_bounds__(256) void decide_recheck_kernel(const T *__restrict__ q, const T *__restrict__ gal,
                                                             const double *__restrict__ thresholds,
                                                             const unsigned long long *__restrict__ counter,
                                                             const uint64_t *__restrict__ cand, int64_t cand_cap,
                                                             uint32_t *__restrict__ out, int64_t W, int64_t *__restrict__ counts)
{
    constexpr int E = PER * 64;
    const int tid = threadIdx.x, m = tid & 15, grp = tid >> 4;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
    if (blockIdx.x == 0 && tid == 0) {
        counts[0] = n;
        counts[1] = (int64_t)nc;
    }
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
        if (live && m == 0 && s >= thresholds[qi]) atomicOr(out + qi * W + (row >> 5), 1u << (row & 31));
    }
}

__global__ __launch_bounds__(256) void row_mask_combine_kernel(const uint32_t *a, const uint32_t *b, int op, int64_t words,
                                                               uint32_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const uint32_t x = a[i], y = b[i];
        out[i] = op == 0 ? (x | y) : (op == 1 ? (x & y) : (x & ~y));
    }
}

// One thread per row, blocks [q * nb, (q + 1) * nb) for query q: the wave's ballots count its 64 rows, the counts stay in
// (wave-uniform) registers over the grid-stride loop and leave with one 64-bit atomicAdd per counter and wave.
__global__ __launch_bounds__(256) void decision_counts_kernel(const uint32_t *__restrict__ masks, int nb, int64_t N,
                                                              const int32_t *__restrict__ labels,
                                                              const int32_t *__restrict__ targets,
                                                              const uint32_t *__restrict__ row_mask,
                                                              unsigned long long *__restrict__ out)
{
    const int q = blockIdx.x / nb, blk = blockIdx.x % nb;
    const int lane = threadIdx.x & 63;
    const int64_t W = (N + 31) >> 5;
    const uint32_t *mrow = masks + (size_t)q * W;
    const int32_t target = labels ? targets[q] : 0;
    unsigned long long tp = 0, fp = 0, pos = 0, neg = 0;
    // whole blocks of rows, so every lane of a wave takes part in every ballot
    for (int64_t r0 = (int64_t)blk * 256; r0 < N; r0 += (int64_t)nb * 256) {
        const int64_t r = r0 + threadIdx.x;
        const bool in = r < N;
        const int64_t w = in ? r >> 5 : 0;
        const bool live = in && (!row_mask || ((row_mask[w] >> (r & 31)) & 1u));
        const bool set = live && ((mrow[w] >> (r & 31)) & 1u);
        const bool same = !labels || labels[in ? r : 0] == target;
        tp += __popcll(__ballot(set && same));
        fp += __popcll(__ballot(set && !same));
        pos += __popcll(__ballot(live && same));
        neg += __popcll(__ballot(live && !same));
    }
    if (lane == 0) {
        if (tp) atomicAdd(out + 4 * q + 0, tp);
        if (fp) atomicAdd(out + 4 * q + 1, fp);
        if (pos) atomicAdd(out + 4 * q + 2, pos);
        if (neg) atomicAdd(out + 4 * q + 3, neg);
    }
}

struct DecidePlan {
    size_t off_cnt, off_nb, off_rb, off_qb, off_qres, off_cand, off_hi, total;
};

static DecidePlan make_decide_plan(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dt, bool need_hi)
{
    DecidePlan p{};
    WsLayout l;
    const int64_t cc = cand_cap > 0 ? cand_cap : 1;
    p.off_cnt = l.take(sizeof(unsigned long long));
    p.off_nb = l.take(sizeof(float));
    p.off_rb = l.take(sizeof(float));
    const bool qsplit = dt == MMR_F32;
    p.off_qb = l.take(qsplit ? (size_t)Q * E * sizeof(bf16_t) : 0);
    p.off_qres = l.take(qsplit ? (size_t)Q * sizeof(float) : 0);
    p.off_cand = l.take((size_t)cc * 8);
    p.off_hi = l.take(dt == MMR_F32 && need_hi ? (size_t)N * E * sizeof(bf16_t) : 0);
    p.total = l.off;
    return p;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_decide_workspace_bytes(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given)
{
    if (N < 0 || Q < 0 || cand_cap < 1 || E < 1 || (dtype != MMR_F32 && dtype != MMR_BF16 && dtype != MMR_F16)) return 0;
    return make_decide_plan(N, E, Q, cand_cap, dtype, !gallery_hi_given).total;
}

extern "C" int mmr_cosine_decide(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                                 int E, const double *thresholds_dev, float gallery_norm_bound,
                                 const float *gallery_norm_bound_dev, const float *resid_bound_dev, const uint32_t *row_mask,
                                 int64_t cand_cap, uint32_t *out_masks, int64_t *counts, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_cosine_decide";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.scan_E(E));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(Q >= 1, "%s: Q=%d must be >= 1", fn, Q);
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_CHECK_ARG(cand_cap >= 1, "%s: cand_cap=%lld must be >= 1", fn, (long long)cand_cap);
    MMR_CHECK_ARG(q != nullptr && thresholds_dev != nullptr, "%s: null pointer (q / thresholds_dev)", fn);
    MMR_CHECK_ARG(counts != nullptr && workspace != nullptr, "%s: null pointer (counts / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && out_masks != nullptr) || N == 0, "%s: null pointer (gallery / out_masks)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)q | (uintptr_t)gallery | (uintptr_t)gallery_hi, "q / gallery / gallery_hi"));
    MMR_CHECK_ARG(((uintptr_t)thresholds_dev & 7) == 0, "%s: thresholds_dev must be 8-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)out_masks & 3) == 0, "%s: out_masks must be 4-byte aligned", fn);
    MMR_TRY(ck.row_mask(row_mask));
    const bool split = dtype == MMR_F32;
    const DecidePlan p = make_decide_plan(N, E, Q, cand_cap, dtype, split && gallery_hi == nullptr);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {       // no rows: no mask words; only the counts are written
        MMR_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
        return MMR_OK;
    }
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
    uint64_t *cand = (uint64_t *)(ws + p.off_cand);

    const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, gallery_norm_bound_dev, (float *)(ws + p.off_nb), st);
    MMR_TRY(nb.rc);
    ScanOperands ops;       // 16-bit rows: bf16, or fp16 for the <f16_t> scan
    MMR_TRY(scan_operands(split, q, Q, gallery, gallery_hi, resid_bound_dev, N, E, (bf16_t *)(ws + p.off_hi),
                          (float *)(ws + p.off_rb), (bf16_t *)(ws + p.off_qb), (float *)(ws + p.off_qres), st, &ops));
    DecideScanArgs a{};
    a.gal = (const bf16_t *)ops.gal;
    a.N = N;
    a.ntiles = (int)((N + RTILE - 1) / RTILE);
    a.thresholds = thresholds_dev;
    a.host_bound = nb.host;
    a.dev_bound = nb.dev;
    a.split = split;
    a.resid_dev = ops.resid;
    a.qres = ops.qres;
    a.counter = counter;
    a.cand = cand;
    a.cand_cap = cand_cap;
    a.row_mask = row_mask;
    a.out = out_masks;
    // every pass holds only live queries' waves (a wave without one stores nothing), and every live query's writer lane
    // stores the word of every tile: all Q * ntiles words are written by the scan, whatever out_masks held
    const int qmax = scan_qmax(E, MMR_BF16);
    const ScanTasks t = scan_tasks(a.ntiles);
    a.tpt = t.tpt;
    for (int q0 = 0; q0 < Q; q0 += qmax) {
        a.q0 = q0;
        a.Qc = (Q - q0) < qmax ? (Q - q0) : qmax;
        a.q = (const bf16_t *)ops.q + (size_t)q0 * E;
        MMR_TRY(dtype == MMR_F16 ? launch_decide_scan<f16_t>(E, a, (unsigned)t.ntasks, st)
                                 : launch_decide_scan<bf16_t>(E, a, (unsigned)t.ntasks, st));
    }

    ProfScope prof(MMR_PROF_FINALIZE, st);
    const dim3 grid(grid_1d(cand_cap, 16, 8192));
    const int64_t W = a.ntiles;
    MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return dispatch_per(E, [&](auto per) -> int {
            hipLaunchKernelGGL((decide_recheck_kernel<T, decltype(per)::value>), grid, dim3(256), 0, st, (const T *)q,
                               (const T *)gallery, thresholds_dev, (const unsigned long long *)counter, (const uint64_t *)cand,
                               cand_cap, out_masks, W, counts);
            return MMR_OK;
        });
    }));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_row_mask_combine(const uint32_t *a, const uint32_t *b, int op, int64_t words, uint32_t *out, void *stream)
{
    MMR_CHECK_ARG(op >= 0 && op <= 2, "mmr_row_mask_combine: op=%d outside {0 (or), 1 (and), 2 (and-not)}", op);
    MMR_CHECK_ARG(words >= 0, "mmr_row_mask_combine: words=%lld must be >= 0", (long long)words);
    if (words == 0) return MMR_OK;
    MMR_CHECK_ARG(a && b && out, "mmr_row_mask_combine: null pointer");
    MMR_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0, "mmr_row_mask_combine: a / b / out must be 4-byte aligned");
    hipLaunchKernelGGL(row_mask_combine_kernel, dim3(grid_1d(words)), dim3(256), 0, (hipStream_t)stream, a, b, op,
                       words, out);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_decision_counts(const uint32_t *masks, int Q, int64_t N, const int32_t *labels, const int32_t *targets,
                                   const uint32_t *row_mask, int64_t *out, void *stream)
{
    const char *fn = "mmr_decision_counts";
    const EntryCheck ck{fn};
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(Q >= 0 && Q <= (1 << 20), "%s: Q=%d outside [0, 2^20]", fn, Q);
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(out != nullptr, "%s: null pointer (out)", fn);
    MMR_CHECK_ARG(masks != nullptr || N == 0, "%s: null pointer (masks)", fn);
    MMR_CHECK_ARG(labels == nullptr || targets != nullptr, "%s: null pointer (targets, with labels given)", fn);
    MMR_CHECK_ARG((((uintptr_t)masks | (uintptr_t)labels | (uintptr_t)targets) & 3) == 0, "%s: masks / labels / targets must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", fn);
    MMR_TRY(ck.row_mask(row_mask));
    hipStream_t st = (hipStream_t)stream;
    MMR_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)Q * 4 * sizeof(int64_t), st));
    if (N == 0) return MMR_OK;
    const int nb = (int)grid_1d(N, 256, 1024);
    hipLaunchKernelGGL(decision_counts_kernel, dim3((unsigned)nb * (unsigned)Q), dim3(256), 0, st, masks, nb, N, labels, targets,
                       row_mask, (unsigned long long *)out);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
