// Arguments of decide_scan_kernel (decide.hip) and its fp16 form (decide_f16.hip).  The kernels' shared body is
// decide_scan_body.inc, included inside each kernel; the geometry is range search's (RangeCfg, range_scan_body.h).
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"
#include "f32_round.h"

#include <math.h>

namespace mmr {

struct DecideScanArgs {
    // 16-bit elements: bf16, or fp16 for decide_scan_f16_kernel (the launcher casts)
    const bf16_t *q;                 // queries of this pass [Qc,E]
    const bf16_t *gal;               // bf16 / fp16 gallery, or the bf16 hi half of an fp32 gallery
    int64_t N;
    int ntiles;                      // = words per mask row
    int Qc;                          // queries in this pass
    int q0;                          // global id of the pass's first query
    int tpt;                         // tiles per task
    const double *thresholds;        // [Q], global query ids, device memory
    float host_bound;                // caller's gallery norm bound (<= 0: none)
    const float *dev_bound;          // measured / caller's device scalar (nullable)
    int split;                       // fp32 gallery scanned through its bf16 hi half
    const float *qres;               // split: ||q - bf16(q)|| per global query
    const float *resid_dev;          // split: max_row ||g - hi|| (nullable: 2^-8 * bound)
    unsigned long long *counter;     // [0] candidates
    uint64_t *cand;
    int64_t cand_cap;
    const uint32_t *row_mask;        // MASKED: rows whose bit is clear never pass (scan_pipeline.h)
    uint32_t *out;                   // [Q, ntiles] mask words
};

// One query's mask word of one tile, stored one tile late (BucketMax's scheme, scan_pipeline.h): flush() runs behind the
// ring's next barrier and ahead of its staging, so the store does not sit between the loads the ring counts.
struct PendingWord {
    uint32_t *row;                   // out + query * ntiles (writer lanes only)
    bool writer;
    uint32_t pend = 0;
    int pend_tile = -1;

    __device__ __forceinline__ void set(int t, uint32_t w) { pend = w; pend_tile = t; }
    __device__ __forceinline__ void flush() {
        if (writer && pend_tile >= 0) row[pend_tile] = pend;
    }
};

}  // namespace mmr
