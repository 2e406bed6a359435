// assign_scan_kernel, the scan of the nearest-centroid assignment (assign.hip), with its arguments and launcher.  One
// kernel template over the element type ET, bf16_t or f16_t (range_scan_body.h says why a template); assign.hip
// instantiates the bf16 kernels, assign_f16.hip the fp16 ones.  The geometry is range search's (RangeCfg).
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"

#include <math.h>

namespace mmr {

constexpr int AGROUP = 32;           // centroids per wave: one GROUP of the per-row triples

struct AssignScanArgs {
    // 16-bit elements: bf16, or fp16 for assign_scan_kernel<f16_t> (the caller casts)
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

// ET: the element type behind a.cen / a.gal.
// range_scan_kernel's non-TRI structure with the MFMA operands swapped (tile_dot_32x32<..., SWAP>): lane (c, h) holds
// tile row c against 16 of the wave's 32 resident centroids, so the reduction over centroids is in-register.
template <typename ET, int E, bool MASKED>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void assign_scan_kernel(AssignScanArgs a)
{
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    const int t0 = blockIdx.x * a.tpt;
    const int t1 = min(a.ntiles, t0 + a.tpt);

    // resident operand: this wave's 32 centroids (scan_kernel's query layout)
    const int lc = wave * AGROUP + c;
    const bool clive = lc < a.Kc;
    const bool compute = wave * AGROUP < a.Kc;            // wave-uniform: this wave holds a live centroid
    // mask words of the tiles [t0, t1): issued in front of the centroid loads, taken behind them (scan_pipeline.h: mask_issue)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    load_query_b16<C::KSTEPS, 16>(a.cen + (size_t)(clive ? lc : 0) * E + h * 8, clive, bq);
    // this lane's 16 centroids are the wave's (i&3) + 8*(i>>2) + 4h: their fp32 biases, -inf for one past K
    float bs[16];
    {
        const float *bp = a.biasf + a.c0 + wave * AGROUP + 4 * h;
#pragma unroll
        for (int i = 0; i < 16; ++i) bs[i] = bp[(i & 3) + 8 * (i >> 2)];
    }
    const uint32_t mwords = mask_take(mw);
    // every load above has landed before the ring starts counting its own (the empty statements need the values)
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) asm volatile("" ::"v"(bq[s]));
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(bs[i]));
    asm volatile("" ::"v"(mwords));

    const size_t plane = (size_t)wave * (size_t)N;
    PendingTriple pt{a.best + plane, a.second + plane, a.arg + plane};

    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.gal, a.gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { pt.flush(); },
        [&](int t, int cur) {
            if (!compute) return;
            const int64_t left = N - (int64_t)t * RTILE;
            const uint32_t lw = MASKED ? row_mask_tile32(mwords, t, t0, N) : (left < 32 ? (1u << (int)left) - 1u : 0xffffffffu);
            if (MASKED && lw == 0u) return;               // wave-uniform: no live row in this tile
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET, true>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(centroid (i&3) + 8*(i>>2) + 4h of the wave, tile row c).  chk turns NaN when a
            // product was NaN or infinite: such a row is not decided here.
            float b = -INFINITY, s2 = -INFINITY, chk = 0.f;
            int bi = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                chk = fmaf(acc[i], 0.f, chk);
                const float v = acc[i] + bs[i];
                s2 = __builtin_amdgcn_fmed3f(b, s2, v);   // s2 <= b: the median is the new runner-up
                bi = v > b ? i : bi;
                b = fmaxf(b, v);
            }
            bi = (bi & 3) + 8 * (bi >> 2) + 4 * h;
            // the other half-wave holds row c against the other 16 centroids
            const float ob = __shfl_xor(b, 32, 64), os2 = __shfl_xor(s2, 32, 64), ochk = __shfl_xor(chk, 32, 64);
            const int obi = __shfl_xor(bi, 32, 64);
            const bool take = ob > b;
            s2 = take ? fmaxf(b, os2) : fmaxf(s2, ob);
            bi = take ? obi : bi;
            b = take ? ob : b;
            chk += ochk;
            const bool store = h == 0 && ((lw >> c) & 1u);
            pt.set(store ? (int64_t)t * RTILE + c : -1, b, s2, chk == 0.f ? a.c0 + wave * AGROUP + bi : -1);
        });
    pt.flush();
}

// a.row_mask NULL: the unmasked kernels
template <typename ET>
int launch_assign_scan(int E, const AssignScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        if (a.row_mask) return launch_scan_kernel<&assign_scan_kernel<ET, decltype(e)::value, true>>(grid, C::THREADS, C::LDS, st, a);
        return launch_scan_kernel<&assign_scan_kernel<ET, decltype(e)::value, false>>(grid, C::THREADS, C::LDS, st, a);
    });
}
// the fp16 kernels: assign_f16.hip
extern template int launch_assign_scan<f16_t>(int, const AssignScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
