// The top-k scans of search.hip (scan_kernel / scan16_kernel for bf16 operands, scan_f32s_kernel for fp32 rows) as a
// host-side call of their own: mmr_cosine_topk's tiers and pass A of the deep top-k (deep_topk.hip).  Defined in search.hip,
// with the gallery norm bound's launch; the rest of the host front end is scan_host.h.
#pragma once
#include "mmr_common.h"

namespace mmr {

// Tile / task geometry of a scan over [N, E] rows: what make_plan gives mmr_cosine_topk.
//   bmax[ntiles][qpad]  maximum of the approximate dots over the live, non-NaN rows of each tile (-inf: none)
//   tmax[ntasks][qpad]  the same per task of tpt tiles
struct TopkScanGeom {
    int tile_rows;      // 32 (bf16 operands) or 16 (fp32 rows)
    int ntiles, tpt, ntasks;
    int qmax;           // queries per pass
};
TopkScanGeom topk_scan_geom(int64_t N, int E, mmr_dtype scan_dtype);

// One pass over the gallery for the Qc <= qmax queries at q; qpad = Qc rounded up to 32.  The one place that picks the scan
// by dtype.  scan_dtype MMR_BF16: q and gal are bf16 (scan_kernel / scan16_kernel); MMR_F16: both fp16 (search_f16.hip: the
// bf16 geometry); MMR_F32: both fp32 -- scan_f32s_kernel over the rows, or, with split_hi / split_lo given
// (mmr_gallery_split_bf16), scan_split_kernel over the split, where `gate` (nullable) is that kernel's second-tier gate.
// row_mask: the packed row mask or NULL.
int launch_topk_scan(mmr_dtype scan_dtype, int E, const void *q, const void *gal, int Qc, int64_t N, const TopkScanGeom &g,
                     int qpad, float *bmax, float *tmax, const uint32_t *row_mask, hipStream_t st,
                     const bf16_t *split_hi = nullptr, const bf16_t *split_lo = nullptr, const int32_t *gate = nullptr);

// ---- a row mask per query (deep_qmask.hip; DESIGN.md section 3, "a row mask per query") ----
// Tiles per task of the per-query scan: the plan's tpt, cut to what the task's mask words [tile][qc + 1] leave room for in
// LDS behind the ring (160 KiB in all); qc: the widest pass's queries, a multiple of 32.  At least 1 for every supported E.
int qmask_scan_tpt(int E, int qc, int tpt);
// launch_topk_scan for bf16 / fp16 operands with one mask row per query: row_masks[Qc][stride] (the pass's first query's row),
// `shared` (nullable) AND-ed in.  tpt from qmask_scan_tpt; same bmax layout, tmax[ceil(ntiles / tpt)][qpad].
int launch_topk_scan_qmasked(mmr_dtype scan_dtype, int E, const void *q, const void *gal, int Qc, int64_t N, int ntiles, int tpt,
                             int qpad, float *bmax, float *tmax, const uint32_t *row_masks, int64_t stride,
                             const uint32_t *shared, hipStream_t st);
// deep_rescore_kernel's launch (deep_topk.hip) with the listed pair's query's mask row AND-ed into the liveness test
int launch_deep_rescore_qmasked(mmr_dtype dtype, int E, const void *q, const void *gal, int64_t N, int tile_rows,
                                const uint32_t *row_mask, const uint32_t *row_masks, int64_t stride, unsigned long long *counter,
                                const uint64_t *tiles, int64_t tile_cap, const double *thr_exact, uint64_t *surv_k,
                                uint64_t *surv_o, int64_t surv_cap, hipStream_t st);

// *out = an fp32 upper bound of the largest row norm of the gallery (0 for N = 0); arguments already checked
// (mmr_gallery_norm_bound is this behind the C ABI's checks)
int launch_norm_bound(const void *gallery, mmr_dtype dtype, int64_t N, int E, float *out, hipStream_t st);

}  // namespace mmr
