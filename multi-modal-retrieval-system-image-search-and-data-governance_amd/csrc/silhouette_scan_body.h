// Geometry and arguments of silhouette_scan_kernel (silhouette.hip) and its fp16 form (silhouette_f16.hip).  The kernels'
// shared body is silhouette_scan_body.inc, included inside each kernel.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"

namespace mmr {

constexpr int SIL_TPC = RTRI_TPC;                 // tiles per chunk: 64 x 32 rows = 2048 fp32 terms per chain, at most
constexpr int SIL_CHUNK_ROWS = SIL_TPC * RTILE;
constexpr int SIL_NORM_LDS = SIL_CHUNK_ROWS * 4;  // the chunk's per-row norm terms, behind the ring's slots

struct SilScanArgs {
    const bf16_t *gal;        // resident operand: the caller's rows [N, E], original order (bf16, or fp16 for the f16 kernel)
    const bf16_t *sorted;     // streamed operand: the label-sorted, tile-padded copy
    int64_t N;
    int64_t spad;             // rows the sorted copy has room for (stage_tile's clamp never bites: chunks hold whole tiles)
    int K;
    int nblk;                 // resident blocks
    const int64_t *start;     // [K + 1] first sorted position of each label
    const int32_t *tstart;    // [K + 1] first tile of each cluster in the sorted copy
    const int32_t *cstart;    // [K + 1] first chunk of each cluster
    const float *nrm;         // [N] per original row: |x|^2 (euclidean) or 1 / |x| (cosine), fp32
    const float *snrm;        // the same per row of the sorted copy
    const int32_t *spos;      // [N] a live row's position in the sorted copy, -1 for a row that is not live
    float *partial;           // [chunks][N]
};

// silhouette_scan_kernel's twin over fp16 elements (silhouette_f16.hip)
int launch_silhouette_scan_f16(int E, int metric, const SilScanArgs &a, unsigned grid, hipStream_t st);

}  // namespace mmr
