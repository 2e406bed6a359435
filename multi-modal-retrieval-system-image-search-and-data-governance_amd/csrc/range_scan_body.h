// range_scan_kernel, the scan of threshold search and the self-join (range.hip), with its geometry, arguments and
// launcher.  One kernel template over the element type ET, bf16_t or f16_t; range.hip instantiates the bf16 kernels,
// range_f16.hip the fp16 ones.
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
    // 16-bit elements: bf16, or fp16 for range_scan_kernel<f16_t> (the caller casts)
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

// ET: the element type behind a.q / a.gal -- it picks the MFMA instruction (scan_pipeline.h) and how the resident query's
// norm is read; everything else is the same for both.  The statements are the kernel's own and not a function the
// bf16 and fp16 kernels call: as an inlined function the bf16 kernels compiled to slightly different instruction streams
// than before the fp16 forms existed (register allocation and scalar-load order); as a kernel template they compile bit
// for bit (profiles/scan_template_isa_diff.txt).
template <typename ET, int E, bool TRI, bool MASKED>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void range_scan_kernel(RangeScanArgs a)
{
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    // work item -> (first query id, tile range)
    int64_t qbase;
    int t0, t1;
    if constexpr (TRI) {
        const int64_t w = blockIdx.x, F = a.fblk;
        int64_t b, ch;
        if (a.order == 0) {
            int64_t lo = 0, hi = a.nchunk - 1;          // largest chunk with S(chunk) <= w
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (tri_items_before_chunk(mid, a.nblk, F) <= w) lo = mid; else hi = mid - 1;
            }
            ch = lo;
            b = w - tri_items_before_chunk(ch, a.nblk, F);
        } else {
            int64_t lo = 0, hi = a.nblk - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (tri_items_before_block(mid, a.nchunk, F) <= w) lo = mid; else hi = mid - 1;
            }
            b = lo;
            ch = b / F + (w - tri_items_before_block(b, a.nchunk, F));
        }
        qbase = b * C::QMAX;
        const int64_t first = qbase / RTILE;          // the tile that holds row b*QMAX
        t0 = (int)max((int64_t)ch * RTRI_TPC, first);
        t1 = (int)min((int64_t)a.ntiles, (int64_t)(ch + 1) * RTRI_TPC);
    } else {
        qbase = a.q0;
        t0 = blockIdx.x * a.tpt;
        t1 = min(a.ntiles, t0 + a.tpt);
    }
    const int64_t nq = TRI ? N : (int64_t)a.q0 + a.Qc;   // query ids below this are live

    // B operand: this wave's 32 queries (scan_kernel's layout)
    const int64_t gq = qbase + wave * 32 + c;
    bool qlive = gq < nq;
    const bool compute = TRI ? qbase + wave * 32 < N : wave * 32 < a.Qc;   // wave-uniform: this wave holds a live query
    // mask words of the tiles [t0, t1) (at most RMAX_TPT / RTRI_TPC = 64) and, in the self-join, the query row's own word:
    // issued in front of the query loads, taken behind them (scan_pipeline.h: mask_issue)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    const MaskWord mq = MASKED && TRI ? mask_issue(a.row_mask, (qlive ? gq : 0) >> 5, 64, 0) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    double qn2 = 0.0;                  // fp64: a small query's squares underflow in fp32
    {
        const bf16_t *qp = TRI ? a.gal + (size_t)(qlive ? gq : 0) * E + h * 8
                               : a.q + (size_t)(qlive ? gq - a.q0 : 0) * E + h * 8;
        load_query_b16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = b16_to_f32<ET>((uint16_t)bq[s][j]); qn2 += x * x; }
    }
    qn2 += __shfl_xor(qn2, 32, 64);
    const uint32_t mwords = mask_take(mw);
    if constexpr (MASKED && TRI) qlive = qlive && ((mask_take(mq) >> (gq & 31)) & 1u);   // a masked query row is not live

    // this lane's candidate threshold: threshold - margin(query) (range_common.h), rounded down to fp32
    float thr;
    bool wild;
    {
        const ScanMargin mg = scan_margin(qn2, a.host_bound, a.dev_bound, a.split, a.resid_dev, a.qres, qlive ? gq : 0);
        wild = mg.wild;
        const double lo = wild ? -INFINITY : a.threshold - mg.eps;
        thr = (float)lo;
        if ((double)thr > lo) thr = nextafterf(thr, -INFINITY);
    }

    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.gal, a.gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [] {},
        [&](int t, int cur) {
            if (!compute) return;
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(query gq, row t*32 + (i&3) + 8*(i>>2) + 4h)
            const int64_t base = (int64_t)t * RTILE + 4 * h;
            const uint32_t wh = MASKED ? row_mask_tile32(mwords, t, t0, N) >> (4 * h) : 0u;
            uint32_t pred = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = base + (i & 3) + 8 * (i >> 2);
                const bool p = qlive && (MASKED ? ((wh >> ((i & 3) + 8 * (i >> 2))) & 1u) : r < N) && (acc[i] >= thr || wild) &&
                               (!TRI || r > gq);
                pred |= p ? (1u << i) : 0u;
            }
            append_candidates(pred, lane, a.counter, a.cand, a.cand_cap, (uint64_t)gq << 32, base);
        });
}

// tri: the self-join's kernels.  a.row_mask NULL: the unmasked kernels.
template <typename ET>
int launch_range_scan(int E, bool tri, const RangeScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        constexpr int EE = decltype(e)::value;
        using C = RangeCfg<EE>;
        if (tri && a.row_mask) return launch_scan_kernel<&range_scan_kernel<ET, EE, true, true>>(grid, C::THREADS, C::LDS, st, a);
        if (tri) return launch_scan_kernel<&range_scan_kernel<ET, EE, true, false>>(grid, C::THREADS, C::LDS, st, a);
        if (a.row_mask) return launch_scan_kernel<&range_scan_kernel<ET, EE, false, true>>(grid, C::THREADS, C::LDS, st, a);
        return launch_scan_kernel<&range_scan_kernel<ET, EE, false, false>>(grid, C::THREADS, C::LDS, st, a);
    });
}
// the fp16 kernels: range_f16.hip
extern template int launch_range_scan<f16_t>(int, bool, const RangeScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
