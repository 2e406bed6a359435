// Geometry, arguments and helpers of range_scan_kernel (range.hip) and its fp16 form (range_f16.hip).  The kernels' shared
// body is range_scan_body.inc, included inside each kernel.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"

#include <math.h>

namespace mmr {

constexpr int RTRI_TPC = 64;             // tiles per self-join chunk (the other scan constants: range_common.h)

// scan_kernel's 32x32 form: E <= 512 runs 8 waves x 32 resident queries, E = 768 4 waves x 32.
template <int E>
struct RangeCfg : Tile32<E> {
    static constexpr int QMAX = Tile32<E>::WAVES * 32;
    static constexpr int KSTEPS = E / 16;
    static constexpr int LDS = RNBUF * Tile32<E>::TILE_BYTES;
};

struct RangeScanArgs {
    // 16-bit elements: bf16, or fp16 for range_scan_f16_kernel (the launcher casts)
    const bf16_t *q;                 // range: queries of this pass [Qc,E]; TRI: the scanned array itself
    const bf16_t *gal;               // bf16 / fp16 gallery, or the bf16 hi half of an fp32 gallery
    int64_t N;
    int ntiles;
    int Qc;                          // range: queries in this pass
    int q0;                          // range: global id of the pass's first query
    int tpt;                         // range: tiles per task
    int nblk, fblk, nchunk, order;   // TRI: query blocks, query blocks per chunk, chunks, 0 = chunk-major / 1 = block-major
    double threshold;
    float host_bound;                // caller's gallery norm bound (<= 0: none)
    const float *dev_bound;          // measured / caller's device scalar (nullable)
    int split;                       // fp32 gallery scanned through its bf16 hi half
    const float *qres;               // split range search: ||q - bf16(q)|| per global query (nullable)
    const float *resid_dev;          // split: max_row ||g - hi|| (nullable: 2^-8 * bound)
    unsigned long long *counter;     // [0] candidates
    uint64_t *cand;
    int64_t cand_cap;
    const uint32_t *row_mask;        // MASKED: rows (and, TRI, query rows) whose bit is clear never pair (scan_pipeline.h)
};

// S(c) = work items of the chunks before c in chunk-major order (chunk c holds the query blocks b < min(nblk, (c+1)F))
__device__ __forceinline__ int64_t tri_items_before_chunk(int64_t c, int64_t nblk, int64_t F)
{
    const int64_t K = nblk / F;
    if (c <= K) return F * c * (c + 1) / 2;
    return F * K * (K + 1) / 2 + (c - K) * nblk;
}
// block-major order: block b holds the chunks c >= b / F
__device__ __forceinline__ int64_t tri_items_before_block(int64_t b, int64_t nchunk, int64_t F)
{
    const int64_t qq = b / F, rr = b % F;
    return b * nchunk - (F * qq * (qq - 1) / 2 + rr * qq);
}

}  // namespace mmr
