// The host front end the scan-based calls share: mmr_cosine_topk* (search.hip), mmr_cosine_range* /
// mmr_gallery_self_join* (range.hip), mmr_threshold_sweep* (sweep.hip), mmr_cosine_topk_deep* (deep_topk.hip,
// deep_qmask.hip), mmr_cosine_decide (decide.hip), mmr_cosine_assign (assign.hip), mmr_silhouette_sums (silhouette.hip)
// and mmr_kmeanspp_seed (kmeanspp.hip); EntryCheck and the dispatchers also serve the row-wise calls (cluster.hip,
// cluster_rank.hip, tip_train.hip, tip_grid.hip).
//   EntryCheck            the argument checks, worded with the entry's name
//   dispatch_elem / _per / _masked   run-time dtype, E and row mask -> template arguments of a kernel launch
//   resolve_norm_bound    the caller's bound, or its device scalar, or a measurement into a workspace slot
//   scan_tasks            tiles per task and task count of a gallery scan
//   scan_operands         the 16-bit operands of an MFMA scan: for an fp32 gallery its bf16 hi half and bf16-rounded queries
// Header-only: nothing here launches a kernel of its own; the launches stay with the kernels' files.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "topk_scan.h"

#include <math.h>
#include <type_traits>

namespace mmr {

// ------------------------------------------------------------------ argument checks
// Every check returns MMR_OK or sets the error, "<entry>: ...", and returns its code.  Entries that word one check in
// two ways keep their wording: the variants are separate members.
struct EntryCheck {
    const char *fn;

    int dtype(mmr_dtype dt) const {
        MMR_CHECK_ARG(dt == MMR_F32 || dt == MMR_BF16 || dt == MMR_F16, "%s: dtype %d", fn, (int)dt);
        return MMR_OK;
    }
    // the MFMA scans' widths (scan_supports_E)
    int scan_E(int E) const {
        if (!scan_supports_E(E)) { set_error("%s: E=%d unsupported (128,256,512,768)", fn, E); return MMR_ENOTSUP; }
        return MMR_OK;
    }
    // row ids are int32: the top-k calls' wording, then the range / sweep calls'
    int sizes_int32(int Q, int64_t N) const {
        MMR_CHECK_ARG(Q >= 0 && N >= 0, "%s: negative size Q=%d N=%lld", fn, Q, (long long)N);
        MMR_CHECK_ARG(N < 0x7fffffff, "%s: N=%lld exceeds int32 row ids (shard the gallery)", fn, (long long)N);
        return MMR_OK;
    }
    int rows_int32(int64_t N) const {
        MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff, "%s: N=%lld outside [0, 2^31-1)", fn, (long long)N);
        return MMR_OK;
    }
    int scale_finite(float scale) const {
        MMR_CHECK_ARG(scale > 0.f && scale < INFINITY, "%s: scale must be finite and > 0 (got %g)", fn, (double)scale);
        return MMR_OK;
    }
    int norm_bound(float b) const {
        MMR_CHECK_ARG(b == b && b < INFINITY, "%s: gallery_norm_bound must be finite", fn);
        return MMR_OK;
    }
    // ptrs: the OR of the operand pointers, named by `what`
    int aligned16(uintptr_t ptrs, const char *what) const {
        MMR_CHECK_ARG((ptrs & 15) == 0, "%s: %s must be 16-byte aligned", fn, what);
        return MMR_OK;
    }
    int row_mask(const uint32_t *words) const {
        MMR_CHECK_ARG(((uintptr_t)words & 3) == 0, "%s: row_mask must be 4-byte aligned", fn);
        return MMR_OK;
    }
    int workspace(size_t have, size_t need) const {
        if (have < need) { set_error("%s: workspace %zu < required %zu", fn, have, need); return MMR_ENOSPC; }
        return MMR_OK;
    }
};

// ------------------------------------------------------------------ dispatch: run-time value -> template argument
// Each calls f with a tag and returns what f returns, in the style of scan_dispatch_E (scan_pipeline.h), which stays the
// dispatcher of the sites that build no E = 1024 variant.
template <class T>
struct ElemTag { using type = T; };

// f(ElemTag<bf16_t | f16_t | float>{}) for a checked dtype
template <class F>
static inline int dispatch_elem(mmr_dtype dt, F &&f)
{
    if (dt == MMR_BF16) return f(ElemTag<bf16_t>{});
    if (dt == MMR_F16) return f(ElemTag<f16_t>{});
    return f(ElemTag<float>{});
}

// f(std::integral_constant<int, PER>{}), PER = E / 64 elements per lane of the exact fp64 dot (exact_dot.h); any other E
// is MMR_ENOTSUP
template <class F>
static inline int dispatch_per(int E, F &&f)
{
    switch (E) {
        case 128: return f(std::integral_constant<int, 2>{});
        case 256: return f(std::integral_constant<int, 4>{});
        case 512: return f(std::integral_constant<int, 8>{});
        case 768: return f(std::integral_constant<int, 12>{});
        case 1024: return f(std::integral_constant<int, 16>{});
        default: set_error("E=%d unsupported (128,256,512,768,1024)", E); return MMR_ENOTSUP;
    }
}

// f(std::bool_constant<row_mask != NULL>{})
template <class F>
static inline int dispatch_masked(const uint32_t *row_mask, F &&f)
{
    return row_mask ? f(std::true_type{}) : f(std::false_type{});
}

// ------------------------------------------------------------------ gallery norm bound
// G of the margins is max(host, *dev).  A caller who gives neither a positive bound nor a device scalar has the gallery
// measured into ws_slot (one extra pass; GalleryIndex-style callers measure once and pass the scalar).
struct NormBound {
    int rc;
    float host;
    const float *dev;
};
static inline NormBound resolve_norm_bound(const void *gallery, mmr_dtype dtype, int64_t N, int E, float caller_bound,
                                           const float *caller_dev, float *ws_slot, hipStream_t st)
{
    NormBound b{MMR_OK, caller_bound > 0.f ? caller_bound : 0.f, caller_dev};
    if (b.host == 0.f && !b.dev) {
        b.rc = launch_norm_bound(gallery, dtype, N, E, ws_slot, st);
        b.dev = ws_slot;
    }
    return b;
}

// ------------------------------------------------------------------ task plan
// Up to SCAN_MAX_TPT tiles per task, about 256 x m tasks: one task per tile up to 256 tiles.
struct ScanTasks {
    int tpt, ntasks;
};
static inline ScanTasks scan_tasks_of(int ntiles, int tpt) { return {tpt, (ntiles + tpt - 1) / tpt}; }
static inline ScanTasks scan_tasks(int ntiles)
{
    if (ntiles <= 256) return scan_tasks_of(ntiles, 1);
    const int m = (ntiles + 256 * SCAN_MAX_TPT - 1) / (256 * SCAN_MAX_TPT);
    return scan_tasks_of(ntiles, (ntiles + 256 * m - 1) / (256 * m));
}

// ------------------------------------------------------------------ operands of a scan that multiplies 16-bit elements
// range.hip: out[Q,E] = bf16(q) (nearest-even) and qres[Q] = ||q - bf16(q)||, rounded up
int range_queries_to_bf16(const float *q, int Q, int E, bf16_t *out, float *qres, hipStream_t st);
// range.hip: hi[N,E] = bf16(g) and *resid = max_row ||g - hi||, rounded up (the call zeroes *resid first)
int range_split_hi(const float *g, int64_t N, int E, bf16_t *hi, float *resid, hipStream_t st);

struct ScanOperands {
    const void *q, *gal;    // what the scan multiplies: bf16 or fp16 elements (or, not split, the caller's own)
    const float *resid;     // split: max_row ||g - hi|| (device scalar, nullable); else NULL
    const float *qres;      // split with queries: ||q - bf16(q)|| per query; else NULL
};
// split = false: the caller's arrays as they are.  split (an fp32 gallery scanned through its bf16 hi half): the gallery
// operand is the caller's gallery_hi with the caller's residual bound, or is built into ws_hi with its bound in ws_rb;
// the queries (q NULL: none, the self-join) are rounded into ws_qb with their residual norms in ws_qres.  The slots are
// the caller's plan's; a slot the case at hand does not use may be NULL.
static inline int scan_operands(bool split, const void *q, int Q, const void *gallery, const void *gallery_hi,
                                const float *resid_dev, int64_t N, int E, bf16_t *ws_hi, float *ws_rb, bf16_t *ws_qb,
                                float *ws_qres, hipStream_t st, ScanOperands *out)
{
    *out = {q, gallery, nullptr, nullptr};
    if (!split) return MMR_OK;
    out->gal = gallery_hi;
    out->resid = resid_dev;
    if (!gallery_hi) {
        MMR_TRY(range_split_hi((const float *)gallery, N, E, ws_hi, ws_rb, st));
        out->gal = ws_hi;
        out->resid = ws_rb;
    }
    if (q) {
        MMR_TRY(range_queries_to_bf16((const float *)q, Q, E, ws_qb, ws_qres, st));
        out->q = ws_qb;
        out->qres = ws_qres;
    }
    return MMR_OK;
}

}  // namespace mmr
