// decide_scan_kernel, the scan of the decision masks (decide.hip), with its arguments and launcher.  One kernel template
// over the element type ET, bf16_t or f16_t (range_scan_body.h says why a template); decide.hip instantiates the bf16
// kernels, decide_f16.hip the fp16 ones.  The geometry is range search's (RangeCfg).
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"
#include "f32_round.h"

#include <math.h>

namespace mmr {

struct DecideScanArgs {
    // 16-bit elements: bf16, or fp16 for decide_scan_kernel<f16_t> (the caller casts)
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

// ET: the element type behind a.q / a.gal.
// range_scan_kernel's non-TRI structure with a deciding epilogue: a 32-row tile is one mask word per query.
template <typename ET, int E, bool MASKED>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void decide_scan_kernel(DecideScanArgs a)
{
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    const int t0 = blockIdx.x * a.tpt;
    const int t1 = min(a.ntiles, t0 + a.tpt);
    const int64_t nq = (int64_t)a.q0 + a.Qc;              // query ids below this are live

    // B operand: this wave's 32 queries (scan_kernel's layout)
    const int64_t gq = (int64_t)a.q0 + wave * 32 + c;
    const bool qlive = gq < nq;
    const bool compute = wave * 32 < a.Qc;                // wave-uniform: this wave holds a live query
    // mask words of the tiles [t0, t1): issued in front of the query loads, taken behind them (scan_pipeline.h: mask_issue)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    double qn2 = 0.0;                  // fp64: a small query's squares underflow in fp32
    {
        const bf16_t *qp = a.q + (size_t)(qlive ? gq - a.q0 : 0) * E + h * 8;
        load_query_b16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = b16_to_f32<ET>((uint16_t)bq[s][j]); qn2 += x * x; }
    }
    qn2 += __shfl_xor(qn2, 32, 64);
    const uint32_t mwords = mask_take(mw);

    // this lane's two thresholds: an approximate dot at or above thr_hi is a certain pass, one below thr_lo a certain
    // fail (|acc - dot64| <= eps: range_common.h), anything else -- NaN included -- is left to the fp64 recheck.  A wild
    // query, or one whose threshold is not finite, leaves every pair to it.
    float thr_lo, thr_hi;
    {
        const ScanMargin mg = scan_margin(qn2, a.host_bound, a.dev_bound, a.split, a.resid_dev, a.qres, qlive ? gq : 0);
        const double thr = a.thresholds[qlive ? gq : 0];
        const bool wild = mg.wild || !(fabs(thr) < INFINITY);
        // a wild lane compares against NaN: no element is a certain pass, none a certain fail, every pair is open
        thr_lo = wild ? NAN : f32_down(thr - mg.eps);
        thr_hi = wild ? NAN : f32_up(thr + mg.eps);
    }

    PendingWord pw{a.out + (size_t)(qlive ? gq : 0) * a.ntiles, compute && qlive && h == 0};

    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.gal, a.gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { pw.flush(); },
        [&](int t, int cur) {
            if (!compute) return;
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(query gq, row t*32 + (i&3) + 8*(i>>2) + 4h), bit (i&3) + 8*(i>>2) + 4h of the word
            const int64_t base = (int64_t)t * RTILE + 4 * h;
            const int64_t left = N - (int64_t)t * RTILE;
            const uint32_t lw = MASKED ? row_mask_tile32(mwords, t, t0, N) : (left < 32 ? (1u << (int)left) - 1u : 0xffffffffu);
            const uint32_t wh = lw >> (4 * h);
            // pass: certain passes; alive: everything but the certain fails (NaN included); both at the rows' bit positions
            uint32_t pass = 0, alive = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t bit = 1u << ((i & 3) + 8 * (i >> 2));
                pass |= acc[i] >= thr_hi ? bit : 0u;
                alive |= acc[i] < thr_lo ? 0u : bit;
            }
            // open pairs of live rows of a live query, moved from bit (i&3) + 8*(i>>2) to bit i for append_candidates
            const uint32_t ob = qlive ? (alive & ~pass & wh) : 0u;
            const uint32_t pred = (ob & 0xfu) | ((ob >> 4) & 0xf0u) | ((ob >> 8) & 0xf00u) | ((ob >> 12) & 0xf000u);
            append_candidates(pred, lane, a.counter, a.cand, a.cand_cap, (uint64_t)gq << 32, base);
            pass <<= 4 * h;
            pass |= __shfl_xor(pass, 32, 64);
            pw.set(t, pass & lw);
        });
    pw.flush();
}

// a.row_mask NULL: the unmasked kernels
template <typename ET>
int launch_decide_scan(int E, const DecideScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        if (a.row_mask) return launch_scan_kernel<&decide_scan_kernel<ET, decltype(e)::value, true>>(grid, C::THREADS, C::LDS, st, a);
        return launch_scan_kernel<&decide_scan_kernel<ET, decltype(e)::value, false>>(grid, C::THREADS, C::LDS, st, a);
    });
}
// the fp16 kernels: decide_f16.hip
extern template int launch_decide_scan<f16_t>(int, const DecideScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
