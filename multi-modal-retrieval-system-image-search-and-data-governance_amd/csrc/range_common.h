// What the thresholded MFMA scans share: range_scan_kernel (range.hip: one threshold, candidate pairs out) and
// sweep_scan_kernel (sweep.hip: a threshold grid, counts out).  Both decide what they can from the approximate dot and
// hand the rest, as (query << 32) | row, to an exact fp64 recheck; the margin that separates the two, the wave prefix
// that compacts the candidates and range search's append to the candidate list live here.  Everything device-side is force-inlined into the kernels.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace mmr {

constexpr int RTILE = 32;                // gallery rows per scan tile
constexpr int RNBUF = 3;                 // LDS ring depth (prefetch distance 2)
constexpr int RPF = 4;                   // k-steps the A fragment reads run ahead of the MFMAs
constexpr int RMAX_TPT = SCAN_MAX_TPT;   // tiles per range-search / sweep task: the top-k scan's (scan_host.h: scan_tasks)
constexpr float R_EPS_REL = 8e-5f;       // MFMA accumulation margin, the one cosine_topk's certificate uses

// margin(query): |acc - dot64| <= eps for every row of the gallery, unless the query is `wild`.
//   qn2         sum of squares of the bf16 query the scan multiplied (fp64: a small query's squares underflow in fp32)
//   host_bound / dev_bound   the gallery norm bound's two sources; G is their maximum
//   split       fp32 gallery scanned through its bf16 hi half: resid_dev = max_row ||g - hi|| (nullable: 2^-8 G),
//               qres[qidx] = ||q - bf16(q)|| (nullable, the self-join: the query is a row, so <= the row residual)
struct ScanMargin {
    double eps;
    bool wild;
};
__device__ __forceinline__ ScanMargin scan_margin(double qn2, float host_bound, const float *dev_bound, int split,
                                                  const float *resid_dev, const float *qres, int64_t qidx)
{
    float G = host_bound > 0.f ? host_bound : 0.f;
    if (dev_bound) G = fmaxf(G, *dev_bound);
    const double qn = sqrt(qn2) * 1.0001;              // ||bf16(q)||, rounded up
    double eps;
    if (split) {
        // the scan multiplied qh = bf16(q) with gh = hi(g): |q.g - qh.gh| <= |q - qh| G + |qh| max|g - gh|, plus the
        // MFMA accumulation error of qh.gh with |gh| <= (1 + 2^-8) G
        const double R = resid_dev ? (double)*resid_dev : 0x1p-8 * (double)G;
        const double qr = qres ? (double)qres[qidx] : R;
        eps = (double)R_EPS_REL * qn * (double)G * (1.0 + 0x1p-8) + qr * (double)G + qn * R;
    } else {
        eps = (double)R_EPS_REL * qn * (double)G;
    }
    eps += 0x1p-137;      // sums in the fp32 subnormal range round absolutely: rank_kernel's term (search.hip)
    // The margin argument needs fp32 accumulations that cannot overflow: every partial sum is at most
    // sum |q_i g_i| <= |q| G, so |q| G < FLT_MAX suffices (1.01: the hi half of an fp32 row is up to 1 + 2^-8 longer, and
    // a value within 2^-8 of FLT_MAX would round to an infinite hi).  Beyond that -- an infinite or NaN norm, or
    // 0 * inf for a zero query against an infinite bound -- an approximate dot may be NaN (inf - inf) or -inf while
    // the exact one is finite: every pair of such a (wild) query is a candidate and the fp64 recheck alone decides.
    const bool wild = !(qn * (double)G * 1.01 < (double)__FLT_MAX__) || !((double)G * 1.01 < (double)__FLT_MAX__);
    return {eps, wild};
}

// Exclusive prefix of the lanes' candidate counts over the wave, and their sum
struct WavePrefix {
    int before, total;
};
__device__ __forceinline__ WavePrefix wave_prefix(int n, int lane)
{
    int incl = n;                                   // inclusive prefix over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        incl += lane >= off ? v : 0;
    }
    return {incl - n, __shfl(incl, 63, 64)};
}

// Append the wave's candidates: bit i of `pred` set = this lane's accumulator element i, i.e. the pair (query of qkey,
// row base + (i&3) + 8*(i>>2)).  Compacted per wave, one 64-bit atomicAdd per wave; the counter keeps counting past the
// list's capacity, the stores stop at it.
__device__ __forceinline__ void append_candidates(uint32_t pred, int lane, unsigned long long *counter, uint64_t *cand,
                                                  int64_t cand_cap, uint64_t qkey, int64_t base)
{
    const WavePrefix wp = wave_prefix(__popc(pred), lane);
    if (wp.total > 0) {
        unsigned long long wbase = 0;
        if (lane == 0) wbase = atomicAdd(counter, (unsigned long long)wp.total);
        wbase = __shfl(wbase, 0, 64);
        unsigned long long pos = wbase + (unsigned long long)wp.before;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (pred & (1u << i)) {
                if (pos < (unsigned long long)cand_cap) cand[pos] = qkey | (uint64_t)(base + (i & 3) + 8 * (i >> 2));
                ++pos;
            }
        }
    }
}

// Host side: the calls that build these scans' operands (range_queries_to_bf16, range_split_hi: range.hip) are declared in
// scan_host.h, next to scan_operands, the one place that calls them.

}  // namespace mmr
