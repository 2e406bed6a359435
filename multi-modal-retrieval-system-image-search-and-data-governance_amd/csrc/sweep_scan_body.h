// Geometry, arguments and helpers of sweep_scan_kernel (sweep.hip) and its fp16 form (sweep_f16.hip).  The kernels' shared
// body is sweep_scan_body.inc, included inside each kernel.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "f32_round.h"

#include <math.h>

namespace mmr {

constexpr int SWEEP_LDS_MAX = 160 * 1024;                        // gfx950: LDS per CU = the most one workgroup can take
constexpr int SWEEP_LABEL_BYTES = RMAX_TPT * RTILE * 4;          // the labels of a task's rows
constexpr int sweep_grid_bytes(int T) { return (2 * (T + 2) * 4 + 15) / 16 * 16; }

// range_scan_kernel's 32x32 form; E = 768 drops to a 2-slot ring (its 3-slot ring would leave 16 KiB for the counts)
template <int E>
struct SweepCfg : Tile32<E> {
    static constexpr int QMAX = Tile32<E>::WAVES * 32;
    static constexpr int KSTEPS = E / 16;
    static constexpr int NBUF = E <= 512 ? RNBUF : 2;
    static constexpr int RING = NBUF * Tile32<E>::TILE_BYTES;
    // queries per pass the kernel can hold: 32 per wave, and the waves' 4 KiB product blocks must fit in one ring slot
    static constexpr int QCAP = (Tile32<E>::TILE_BYTES / 4096 < Tile32<E>::WAVES ? Tile32<E>::TILE_BYTES / 4096 : Tile32<E>::WAVES) * 32;
    static constexpr int FIXED_MAX = RING + SWEEP_LABEL_BYTES + sweep_grid_bytes(MMR_SWEEP_T_MAX);
    // at the largest grid at least 8 queries fit beside the ring
    static_assert(FIXED_MAX + 512 + 8 * (MMR_SWEEP_T_MAX + 1) * 4 + Tile32<E>::WAVES * 32 * 8 <= SWEEP_LDS_MAX,
                  "sweep LDS layout exceeds 160 KiB");
};

constexpr int SWEEP_STAGE_MIN = 32;      // candidate staging every wave is guaranteed, in entries
constexpr int SWEEP_STAGE_MAX = 4096;

struct SweepScanArgs {
    // 16-bit elements: bf16, or fp16 for sweep_scan_f16_kernel (the launcher casts)
    const bf16_t *q;                 // queries of this pass [Qc,E]
    const bf16_t *gal;               // bf16 / fp16 gallery, or the bf16 hi half of an fp32 gallery
    int64_t N;
    int ntiles;
    int Qc;                          // queries in this pass
    int q0;                          // global id of the pass's first query
    int tpt;                         // tiles per task
    float host_bound;                // caller's gallery norm bound (<= 0: none)
    const float *dev_bound;          // measured / caller's device scalar (nullable)
    int split;                       // fp32 gallery scanned through its bf16 hi half
    const float *qres;               // split: ||q - bf16(q)|| per global query
    const float *resid_dev;          // split: max_row ||g - hi|| (nullable: 2^-8 * bound)
    unsigned long long *counter;     // [0] candidates
    uint64_t *cand;
    int64_t cand_cap;
    const uint32_t *row_mask;        // MASKED: rows whose bit is clear are counted nowhere
    const int32_t *labels;           // [N]
    const int32_t *targets;          // [Q], global query ids
    const float *grid32;             // down[T+2] then up[T+2] (sweep_grid_kernel)
    int T;
    int hrows;                       // histogram rows in LDS (>= Qc)
    int ncw;                         // waves that multiply in this pass: ceil(Qc / 32)
    int stage;                       // candidate staging entries per wave, behind the histogram
    float gt0, ginv;                 // bin guess for evenly spaced grids: (x - gt0) * ginv
    unsigned long long *hist;        // [Q,2,T+1] global counts
};

// f32_down / f32_up, (float)x rounded toward -inf / +inf: f32_round.h

// Append the `n` candidates a wave staged in LDS: one atomicAdd, the lanes copy
__device__ __forceinline__ void flush_staged(const uint64_t *stg, int n, int lane, unsigned long long *counter, uint64_t *cand,
                                             int64_t cand_cap)
{
    if (n == 0) return;
    unsigned long long wbase = 0;
    if (lane == 0) wbase = atomicAdd(counter, (unsigned long long)n);
    wbase = __shfl(wbase, 0, 64);
    for (int i = lane; i < n; i += 64) {
        const unsigned long long pos = wbase + (unsigned long long)i;
        if (pos < (unsigned long long)cand_cap) cand[pos] = stg[i];
    }
}

}  // namespace mmr
