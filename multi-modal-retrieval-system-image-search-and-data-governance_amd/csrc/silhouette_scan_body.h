// silhouette_scan_kernel, the pairwise scan of the silhouette sums (silhouette.hip), with its geometry, arguments and
// launcher.  One kernel template over the element type ET, bf16_t or f16_t (range_scan_body.h says why a template);
// silhouette.hip instantiates the bf16 kernels, silhouette_f16.hip the fp16 ones.
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
    const bf16_t *gal;        // resident operand: the caller's rows [N, E], original order (bf16, or fp16 for the <f16_t> kernel)
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

// ET: the element type behind a.gal / a.sorted.
// Work item (chunk ch, resident block b): the distances of the block's rows -- original order, live or not -- to the rows
// of one chunk of the sorted copy, all of one cluster, summed per resident row in one fp32 register per lane.  Nothing is
// loaded inside the ring: the chunk's norm terms are staged in LDS in front of it, the self pair is found by position and
// the padding rows by count.
template <typename ET, int E, bool COS>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void silhouette_scan_kernel(SilScanArgs a)
{
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *nlds = reinterpret_cast<float *>(smem + C::LDS);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    // blockIdx -> (chunk, resident block): neighbouring workgroups stream the same chunk
    const int ch = (int)(blockIdx.x / (unsigned)a.nblk), b = (int)(blockIdx.x % (unsigned)a.nblk);
    if (ch >= a.cstart[a.K]) return;                       // the grid is sized for the worst labelling
    int lo = 0, hi = a.K - 1;                              // the cluster of chunk ch: the first k with cstart[k + 1] > ch
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cstart[mid + 1] > ch) hi = mid; else lo = mid + 1;
    }
    const int k = lo;
    const int tk = a.tstart[k];
    const int t0 = tk + (ch - a.cstart[k]) * SIL_TPC;
    const int t1 = min(a.tstart[k + 1], t0 + SIL_TPC);
    const int64_t rows_k = a.start[k + 1] - a.start[k];    // the cluster's live rows; the rest of its last tile is padding

    // B operand: this wave's 32 resident rows
    const int64_t qbase = (int64_t)b * C::QMAX;
    const int64_t gq = qbase + wave * 32 + c;
    const bool qlive = gq < N;
    const bool compute = qbase + wave * 32 < N;            // wave-uniform
    bf16x8 bq[C::KSTEPS];
    load_query_b16<C::KSTEPS, 16>(a.gal + (size_t)(qlive ? gq : 0) * E + h * 8, qlive, bq);
    const float ni = a.nrm[qlive ? gq : 0];
    const int sp = a.spos[qlive ? gq : 0];

    for (int i = threadIdx.x; i < (t1 - t0) * RTILE; i += C::THREADS) nlds[i] = a.snrm[(size_t)t0 * RTILE + i];
    __syncthreads();

    float run = 0.f;
    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.sorted, a.sorted, a.spad, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [] {},
        [&](int t, int cur) {
            if (!compute) return;
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(resident row gq, sorted row t*32 + (i&3) + 8*(i>>2) + 4h)
            const float *nt = nlds + (t - t0) * RTILE + 4 * h;
            auto dist = [&](float x, float nj) -> float {
                if constexpr (COS) {
                    return 1.f - x * ni * nj;
                } else {
                    float d2 = fmaf(-2.f, x, ni + nj);
                    d2 = d2 < 0.f ? 0.f : d2;              // a select, not a max: NaN stays NaN
                    return __builtin_amdgcn_sqrtf(d2);
                }
            };
            const int64_t left = rows_k - (int64_t)(t - tk) * RTILE;   // live rows from this tile on
            const int rel = sp - t * RTILE - 4 * h;                    // the lane's own row, as an offset into its 16
            const bool self_here = sp >= 0 && rel >= 0 && rel < 28;
            if (left >= RTILE && !__any(self_here)) {                  // wave-uniform: a full tile without a self pair
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 nj = *reinterpret_cast<const float4 *>(nt + 8 * g);
                    run += dist(acc[4 * g + 0], nj.x);
                    run += dist(acc[4 * g + 1], nj.y);
                    run += dist(acc[4 * g + 2], nj.z);
                    run += dist(acc[4 * g + 3], nj.w);
                }
            } else {
                // bit o set: the lane's element at offset o is a live row of the cluster and not the lane's own row
                const int lim = (int)(left < RTILE ? left : RTILE) - 4 * h;
                uint32_t ok = lim >= 28 ? 0x0f0f0f0fu : (lim <= 0 ? 0u : 0x0f0f0f0fu & ((1u << lim) - 1u));
                if (self_here) ok &= ~(1u << rel);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 nj = *reinterpret_cast<const float4 *>(nt + 8 * g);
                    const float njv[4] = {nj.x, nj.y, nj.z, nj.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) run += ((ok >> (8 * g + j)) & 1u) ? dist(acc[4 * g + j], njv[j]) : 0.f;
                }
            }
        });

    run += __shfl_xor(run, 32, 64);
    if (compute && qlive && h == 0) a.partial[(size_t)ch * (size_t)N + (size_t)gq] = run;
}

// metric: 0 = euclidean, 1 = cosine
template <typename ET>
int launch_silhouette_scan(int E, int metric, const SilScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        constexpr int lds = C::LDS + SIL_NORM_LDS;
        if (metric) return launch_scan_kernel<&silhouette_scan_kernel<ET, decltype(e)::value, true>>(grid, C::THREADS, lds, st, a);
        return launch_scan_kernel<&silhouette_scan_kernel<ET, decltype(e)::value, false>>(grid, C::THREADS, lds, st, a);
    });
}
// the fp16 kernels: silhouette_f16.hip
extern template int launch_silhouette_scan<f16_t>(int, int, const SilScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
