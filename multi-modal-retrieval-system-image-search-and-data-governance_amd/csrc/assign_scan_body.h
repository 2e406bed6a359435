// Arguments of assign_scan_kernel (assign.hip) and its fp16 form (assign_f16.hip).  The kernels' shared body is
// assign_scan_body.inc, included inside each kernel; the geometry is range search's (RangeCfg, range_scan_body.h).
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"

#include <math.h>

namespace mmr {

constexpr int AGROUP = 32;           // centroids per wave: one GROUP of the per-row triples

struct AssignScanArgs {
    // 16-bit elements: bf16, or fp16 for assign_scan_f16_kernel (the launcher casts)
    const bf16_t *cen;               // centroids of this pass [Kc,E]
    const bf16_t *gal;               // bf16 / fp16 gallery
    int64_t N;
    int ntiles;
    int Kc;                          // centroids in this pass
    int c0;                          // global id of the pass's first centroid (a multiple of AGROUP)
    int tpt;                         // tiles per task
    const float *biasf;              // [groups * AGROUP] fp32 bias by global centroid id; -inf past K (assign_prep_kernel)
    const uint32_t *row_mask;        // MASKED: rows whose bit is clear are not stored; a tile without a live row is skipped
    // the pass's per-(wave, row) triples, [WAVES][N] each: best approximate score, runner-up, centroid id (-1: a product
    // of this row was not finite, the row goes to the recheck)
    float *best, *second;
    int32_t *arg;
};

// One wave's triple of one tile row, stored one tile late (BucketMax's scheme, scan_pipeline.h): flush() runs behind the
// ring's next barrier and ahead of its staging, so the stores do not sit between the loads the ring counts.
struct PendingTriple {
    float *best, *second;            // the wave's planes
    int32_t *arg;
    float b = 0.f, s = 0.f;
    int32_t a = 0;
    int64_t row = -1;                // < 0: nothing pending (or a lane that does not store)

    __device__ __forceinline__ void set(int64_t r, float b_, float s_, int32_t a_) { row = r; b = b_; s = s_; a = a_; }
    __device__ __forceinline__ void flush() {
        if (row >= 0) { best[row] = b; second[row] = s; arg[row] = a; }
        row = -1;
    }
};

}  // namespace mmr
