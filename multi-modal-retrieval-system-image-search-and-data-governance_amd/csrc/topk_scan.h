// The top-k scans of search.hip (scan_kernel / scan16_kernel for bf16 operands, scan_f32s_kernel for fp32 rows) as a
// host-side call of their own: pass A of the deep top-k (deep_topk.hip).  Defined in search.hip.
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

// One pass over the gallery for the Qc <= qmax queries at q; qpad = Qc rounded up to 32.  scan_dtype MMR_BF16: q and gal
// are bf16; MMR_F16: both fp16 (search_f16.hip: the bf16 geometry); MMR_F32: both fp32.  row_mask: the packed row mask or NULL.
int launch_topk_scan(mmr_dtype scan_dtype, int E, const void *q, const void *gal, int Qc, int64_t N, int qpad, float *bmax,
                     float *tmax, const uint32_t *row_mask, hipStream_t st);

}  // namespace mmr
