// Cosine / dot-product top-k over a gallery matrix for gfx950 (MI355X).
//
// Replaces the reference's scoring + ranking expressions
//     similarity = 100. * features @ ref_feature.t()     reference code/search_image.py:107
//     output.topk(k, 1, True, True)                       reference code/utils.py:17
// generalised to Q query rows.  The [Q,N] score matrix is never
// written.
//
// Structure (DESIGN.md "search"):
//   scan_kernel      HBM-bound.  Streams the bf16 gallery once through LDS (scan_pipeline.h: global_load_lds,
//                    3-deep ring, counted vmcnt, raw s_barrier), multiplies each 32-row tile with
//                    up to 256 register-resident queries on v_mfma_f32_32x32x16_bf16 and keeps only
//                    the per-(query, tile) maximum ("bucket max") and per-(query, task) maximum.
//                    fp16 galleries: the same scan on v_mfma_f32_32x32x16_f16 (the kernel is a template over the element
//                    type, topk_scan_body.h; search_f16.hip compiles the fp16 ones), same bucket maxima layout, same finalize.
//   finalize_kernel  one workgroup per query: picks the KS best tasks, then the KS best tiles inside
//                    them, then re-scores those KS*32 rows EXACTLY (fp64, fixed summation order
//                    shared with oracle/search_ref.c) and orders them by (-dot, +row).  It certifies
//                    that no excluded tile could hold a top-k row; uncertified queries are flagged.
//   exh_* kernels    exhaustive exact fp64 path: fp32 galleries, unsupported E / large k, and any
//                    query the certificate rejected.  Launched unconditionally; unflagged queries
//                    exit at once, so there is no host round trip.
// Why this is exact: every row with dot >= (k-th best dot) lives in a tile whose max is >= that
// value; at most KS tiles can have such a max unless more than KS-k rows are within the MFMA
// rounding error of the k-th -- which is exactly what the certificate checks.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "topk_scan.h"
#include "topk_scan_body.h"
#include "scan_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace mmr {

constexpr int TILE_ROWS_F32 = 16;
constexpr int MAX_TPT = SCAN_MAX_TPT;       // tiles per task
constexpr int KS_MAX = 32;                  // candidate tiles kept per query
constexpr int K_MAX = 64;                   // largest k (exhaustive path)
constexpr int FIN_THREADS = 256;

__host__ __device__ static inline bool ranks_before(double sa, int64_t ia, double sb, int64_t ib) {
    return sa > sb || (sa == sb && ia < ib);
}

// scan_kernel (E <= 512), scan16_kernel (E = 768) and launch_topk_scan_16, the scans over bf16 / fp16 operands:
// topk_scan_body.h.  The fp16 kernels are compiled in search_f16.hip.

// ---------------------------------------------------------------------------------------------
// scan for fp32 galleries at the bf16 MFMA rate: split-bf16.  Every fp32 value x is split into hi = bf16(x) and
// lo = bf16(x - hi) (bf16 keeps 8 significand bits: |x - hi| <= 2^-8 |x|, so x = hi + lo up to 2^-16 |x|) and the dot product
// is accumulated as q_hi.g_hi + q_lo.g_hi + q_hi.g_lo on v_mfma_f32_16x16x32_bf16 (tile_dot_split3) -- three MFMAs per 32-deep
// k-step instead of the eight v_mfma_f32_16x16x4_f32 (1/16 of the bf16 rate) an fp32-MFMA scan needs.  Error of the approximate
// dot against the exact one: the dropped q_lo.g_lo and the two representation residuals, 3 * 2^-16 |q||g| = 4.6e-5 in the worst
// case (1e-5 typical), plus fp32 accumulation (a 32-term tree per MFMA, then E/32 chained adds: <= ~30 * 2^-24 = 2e-6): inside
// the certificate's 8e-5 |q||g| margin, and the ranking itself is still done on exact fp64 re-scores.
// Per 16-row tile: the fp32 rows arrive by global_load_lds (ring of NBUF tiles); ALL waves then split the tile ONCE into
// two bf16 images (hi, lo; 24 VALU instructions per 8 values -- done per consuming wave instead, the conversion was 8x
// redundant and the kernel VALU-bound: 0.78 ms for 1M x 512 x 128 queries); the computing waves read their A fragments
// from those images exactly like scan16_kernel (conflict-free ds_read_b128, prefetched with counted lgkmcnt waits).
// Each wave keeps 16 queries resident as hi/lo B fragments.
//   conversion unit (row = id & 15, cg = id >> 4): fp32 chunks 4cg .. 4cg+3 of the row -> bf16 chunks 2cg, 2cg+1 of both
//   images; a 16-lane group works on 16 different rows at one chunk index, so slot = (chunk ^ row) & 15 is a bijection
//   for its reads and its writes.
// ---------------------------------------------------------------------------------------------
template <int E>
struct ScanF32sCfg : TileGeom<E, 4, TILE_ROWS_F32, E <= 512 ? 8 : 4> {  // E = 768: 192 VGPRs of resident queries -> one wave per SIMD
    using G = TileGeom<E, 4, TILE_ROWS_F32, E <= 512 ? 8 : 4>;
    // scan_split_kernel's ring slot: the hi and the lo bf16 image of one tile, 16 rows each (the bytes of the fp32 tile)
    using Split = TileGeom<E, 2, 2 * TILE_ROWS_F32, G::WAVES>;
    static constexpr int IMG_BYTES = G::TILE_BYTES / 2;    // one bf16 image (hi or lo)
    static constexpr int QMAX = G::WAVES * 16;
    static constexpr int NBUF = E <= 512 ? 3 : 2;          // fp32 tiles in the ring (E = 768: 48 KiB each)
    static constexpr int KSTEPS = E / 32;
    static constexpr int UNITS = TILE_ROWS_F32 * (E / 16); // conversion units per tile
    static constexpr int LDS = NBUF * G::TILE_BYTES + 2 * IMG_BYTES;           // E = 512: 96 + 32 KiB
    static constexpr int SPLIT_LDS = NBUF * G::TILE_BYTES;                     // scan_split_kernel: the ring alone
    static_assert(Split::TILE_BYTES == G::TILE_BYTES && Split::LPW == G::LPW, "a split slot is the bytes of an fp32 tile");
};

template <int E, bool MASKED>
__global__ __launch_bounds__(ScanF32sCfg<E>::THREADS, ScanF32sCfg<E>::WAVES / 4) void scan_f32s_kernel(
    const float *__restrict__ q, const float *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt, int qwaves,
    int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask)
{
    using C = ScanF32sCfg<E>;
    constexpr int IMG_BYTES = C::IMG_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *img = smem + C::NBUF * C::TILE_BYTES;          // [hi | lo] bf16 images of the tile being multiplied
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int task = blockIdx.x;
    const int t0 = task * tpt;
    const int t1 = min(ntiles, t0 + tpt);
    const bool compute = wave < qwaves;

    // 16-row tiles: the words of tiles [t0, t1) start at word t0 / 2
    const MaskWord mw = MASKED ? mask_issue(row_mask, t0 >> 1, ((t1 - 1) >> 1) - (t0 >> 1) + 1, lane) : MaskWord{0u, false};
    bf16x8 bqh[C::KSTEPS], bql[C::KSTEPS];     // query (wave*16 + r), elements [32s + 8g, +8), split
    {
        const int qrow = wave * 16 + r;
        const bool live = compute && qrow < Q;
        load_query_split<C::KSTEPS>(q + (size_t)(live ? qrow : 0) * E + g * 8, live, bqh, bql);
    }
    const uint32_t mwords = mask_take(mw);

    // split the fp32 tile in ring slot `slot` into the hi / lo bf16 images, once for the whole workgroup.  The LDS
    // accesses are inline asm: for C++ accesses hipcc orders them behind the LDS-DMA in flight with s_waitcnt vmcnt(0)
    // (seen in the ISA), which would expose one HBM latency per tile.
    auto convert = [&](int slot) {
        typedef float f32x4_raw __attribute__((ext_vector_type(4)));
        const uint32_t tf = (uint32_t)(uintptr_t)(smem + slot * C::TILE_BYTES);
        const uint32_t ih = (uint32_t)(uintptr_t)img, il = ih + IMG_BYTES;
#pragma unroll
        for (int u = threadIdx.x; u < C::UNITS; u += C::THREADS) {
            const int row = u & 15, cg = u >> 4;
            f32x4_raw x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t a = tf + row * C::ROWB + (swizzle(4 * cg + j, row) << 4);
                asm volatile("ds_read_b128 %0, %1" : "=v"(x[j]) : "v"(a));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bf16x8 hi, lo;
                split_bf16x8(make_float4(x[2 * j][0], x[2 * j][1], x[2 * j][2], x[2 * j][3]),
                             make_float4(x[2 * j + 1][0], x[2 * j + 1][1], x[2 * j + 1][2], x[2 * j + 1][3]), hi, lo);
                const uint32_t off = row * (E * 2) + (swizzle(2 * cg + j, row) << 4);
                asm volatile("ds_write_b128 %0, %1" ::"v"(ih + off), "v"(hi) : "memory");
                asm volatile("ds_write_b128 %0, %1" ::"v"(il + off), "v"(lo) : "memory");
            }
        }
    };

    // split, barrier, multiply: two barriers per tile.  A second image pair with tile t+1 split while tile t is multiplied
    // (one barrier per tile, also with the two waves of a SIMD taking the two jobs in opposite orders) measured no faster:
    // 0.62 vs 0.60 ms for 1M x 512 x 128 queries -- and needs the whole 160 KiB of LDS at E = 512.
    // The ring's barrier also tells that every wave is done reading the bf16 images of tile t-1.
    BucketMax bm{bmax, qpad, wave * 16 + r, compute, g == 0};
    tile_ring<C::NBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(gal, gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { bm.flush(); },
        [&](int t, int cur) {
            convert(cur);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();           // the images are complete
            if (compute)
                bm.add(t, tile_max_16<MASKED>(tile_dot_split3<E>(img, img + IMG_BYTES, r, g, bqh, bql), t, N, g,
                                              MASKED ? row_mask_tile16(mwords, t, t0, N) : 0u));
        });
    bm.finish(tmax, task);
}

// ---------------------------------------------------------------------------------------------
// fp32 galleries that are searched many times (GalleryIndex): the hi / lo split of the gallery is done ONCE, into two bf16
// arrays (together the bytes of the fp32 gallery), and the scan streams those.  scan_f32s_kernel spends its time above the
// HBM stream on the split itself: 24 VALU instructions per 8 values, the images' LDS writes and a second barrier per tile
// (0.60 ms for 1M x 512 x 128 queries against 0.35 ms of HBM time); here a tile arrives by LDS-DMA already as the two
// images scan_f32s builds, there is one barrier per tile, and what is left is the three MFMAs per k-step.  Same split
// function, hence the same MFMA operands, the same bucket maxima and the same candidates; the exact re-score still reads
// the fp32 gallery.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split_gallery_kernel(const float *__restrict__ g, int64_t n8, bf16_t *__restrict__ hi,
                                                            bf16_t *__restrict__ lo)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one unit = 8 consecutive values
    if (i >= n8) return;
    const float4 a0 = *reinterpret_cast<const float4 *>(g + i * 8), a1 = *reinterpret_cast<const float4 *>(g + i * 8 + 4);
    bf16x8 h, l;
    split_bf16x8(a0, a1, h, l);
    *reinterpret_cast<bf16x8 *>(hi + i * 8) = h;
    *reinterpret_cast<bf16x8 *>(lo + i * 8) = l;
}

// fp32 queries rounded to bf16 (nearest-even, the gallery split's hi): operands of the first-tier scan.  One wave per query;
// qres[query] = ||q - bf16(q)||_2, rounded up: the query half of that tier's certificate margin.
__global__ __launch_bounds__(256) void queries_to_bf16_kernel(const float *__restrict__ q, int Q, int E, bf16_t *__restrict__ out,
                                                              float *__restrict__ qres)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Q) return;
    const float *p = q + (size_t)row * E;
    double ss = 0.0;                       // fp64: the squares of a small query's residuals underflow in fp32
    for (int c = lane; c < E / 8; c += 64) {
        const float4 a0 = *reinterpret_cast<const float4 *>(p + c * 8), a1 = *reinterpret_cast<const float4 *>(p + c * 8 + 4);
        const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        union { bf16x8 v; uint32_t u[4]; } h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h.u[j] = pack_bf16x2(x[2 * j], x[2 * j + 1]);
            const double r0 = x[2 * j] - __uint_as_float(h.u[j] << 16);            // exact: the residual of a rounding
            const double r1 = x[2 * j + 1] - __uint_as_float(h.u[j] & 0xffff0000u);
            ss += r0 * r0 + r1 * r1;
        }
        *reinterpret_cast<bf16x8 *>(out + (size_t)row * E + c * 8) = h.v;
    }
    ss = wave_sum_f64_butterfly(ss);
    if (lane == 0) qres[row] = norm_upper_f32(ss, 1.00001f);
}

template <int E, bool MASKED>
__global__ __launch_bounds__(ScanF32sCfg<E>::THREADS, ScanF32sCfg<E>::WAVES / 4) void scan_split_kernel(
    const float *__restrict__ q, const bf16_t *__restrict__ ghi, const bf16_t *__restrict__ glo, int Q, int64_t N, int ntiles,
    int tpt, int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const int32_t *__restrict__ gate,
    const uint32_t *__restrict__ row_mask)
{
    using C = ScanF32sCfg<E>;
    if (gate) {                              // second tier: nothing to do unless the first tier left one of these queries open
        int open = 0;
        for (int i = threadIdx.x; i < Q; i += blockDim.x) open |= gate[i];
        if (!__syncthreads_or(open)) return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int task = blockIdx.x;
    const int t0 = task * tpt;
    const int t1 = min(ntiles, t0 + tpt);
    const bool compute = wave < qwaves;

    const MaskWord mw = MASKED ? mask_issue(row_mask, t0 >> 1, ((t1 - 1) >> 1) - (t0 >> 1) + 1, lane) : MaskWord{0u, false};
    bf16x8 bqh[C::KSTEPS], bql[C::KSTEPS];     // query (wave*16 + r), elements [32s + 8g, +8), split
    {
        const int qrow = wave * 16 + r;
        const bool live = compute && qrow < Q;
        load_query_split<C::KSTEPS>(q + (size_t)(live ? qrow : 0) * E + g * 8, live, bqh, bql);
    }
    const uint32_t mwords = mask_take(mw);
    // one ring slot = [hi image | lo image], each [16 rows][E bf16] with scan_f32s' chunk swizzle, lane-linear for LDS-DMA.
    // A fourth ring slot and fragment reads six k-steps ahead both measured no faster.
    BucketMax bm{bmax, qpad, wave * 16 + r, compute, g == 0};
    tile_ring<C::NBUF, C::LPW>(
        t0, t1,
        [&](int tile, int buf) { stage_tile<typename C::Split, 2>(ghi, glo, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { bm.flush(); },
        [&](int t, int cur) {
            const char *img_hi = smem + cur * C::TILE_BYTES;
            if (compute)
                bm.add(t, tile_max_16<MASKED>(tile_dot_split3<E>(img_hi, img_hi + C::IMG_BYTES, r, g, bqh, bql), t, N, g,
                                              MASKED ? row_mask_tile16(mwords, t, t0, N) : 0u));
        });
    bm.finish(tmax, task);
}

// exact fp64 dot (load_chunk, chunk_partial, exact_dot, QuadQuery / QuadRow / quad_dot): exact_dot.h

// ---------------------------------------------------------------------------------------------
// selection: extract the best (value, key) pairs in (-value, +key) order
// ---------------------------------------------------------------------------------------------
#ifndef MMR_SEL_THRESH
#define MMR_SEL_THRESH 1          // -DMMR_SEL_THRESH=0: serial extraction everywhere (A/B build)
#endif
constexpr int32_t KEY_NONE = 0x7fffffff;
constexpr int SEL_R = 16;                       // candidates per lane in the register path
constexpr int SEL_FAST_MAX = SEL_R * FIN_THREADS;  // 4096

template <typename V, typename K>
__device__ __forceinline__ bool before(V sa, K ia, V sb, K ib) { return sa > sb || (sa == sb && ia < ib); }

template <typename V>
struct SelScratch {
    V pv[FIN_THREADS / 64][K_MAX + 1];
    int32_t pk[FIN_THREADS / 64][K_MAX + 1];
    V bv;
    int32_t bk;
};

// ---- branch-free candidate keys.  A candidate (value, key) becomes an unsigned sort key whose MAXIMUM is the
// best candidate in (-value, +key) order: high part = order-preserving bits of the value, low part = ~key.
// Empty slots are all-zero (below every real candidate: real low parts are >= 1 because key < KEY_NONE).
// ord_f32 / ord_f64 and their inverses: mmr_common.h

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
// DPP controls: quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror: four steps that leave the
// maximum of each 16-lane row in all of its lanes (plain VALU, no LDS round trip); rows are then merged
// with two cross-row shuffles.
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

struct Key64 {    // float value
    uint64_t k;
    __device__ __forceinline__ static Key64 make(float v, int32_t key) { return {((uint64_t)ord_f32(v) << 32) | (uint32_t)~(uint32_t)key}; }
    __device__ __forceinline__ static Key64 none() { return {0}; }
    __device__ __forceinline__ bool empty() const { return k == 0; }
    __device__ __forceinline__ void take_max(const Key64 &o) { k = o.k > k ? o.k : k; }
    __device__ __forceinline__ bool same(const Key64 &o) const { return k == o.k; }
    template <int CTRL> __device__ __forceinline__ Key64 via_dpp() const {
        return {((uint64_t)dpp<CTRL>((uint32_t)(k >> 32)) << 32) | dpp<CTRL>((uint32_t)k)};
    }
    __device__ __forceinline__ Key64 via_xor(int off) const { return {(uint64_t)__shfl_xor((unsigned long long)k, off, 64)}; }
    __device__ __forceinline__ float value() const { return unord_f32((uint32_t)(k >> 32)); }
    __device__ __forceinline__ int32_t key() const { return (int32_t)~(uint32_t)k; }
};
struct Key96 {    // double value
    uint64_t hi; uint32_t lo;
    __device__ __forceinline__ static Key96 make(double v, int32_t key) { return {ord_f64(v), (uint32_t)~(uint32_t)key}; }
    __device__ __forceinline__ static Key96 none() { return {0, 0}; }
    __device__ __forceinline__ bool empty() const { return (hi | lo) == 0; }
    __device__ __forceinline__ void take_max(const Key96 &o) {
        const bool t = (o.hi > hi) | ((o.hi == hi) & (o.lo > lo));
        hi = t ? o.hi : hi; lo = t ? o.lo : lo;
    }
    __device__ __forceinline__ bool same(const Key96 &o) const { return (hi == o.hi) & (lo == o.lo); }
    template <int CTRL> __device__ __forceinline__ Key96 via_dpp() const {
        return {((uint64_t)dpp<CTRL>((uint32_t)(hi >> 32)) << 32) | dpp<CTRL>((uint32_t)hi), dpp<CTRL>(lo)};
    }
    __device__ __forceinline__ Key96 via_xor(int off) const {
        return {(uint64_t)__shfl_xor((unsigned long long)hi, off, 64), (uint32_t)__shfl_xor((int)lo, off, 64)};
    }
    __device__ __forceinline__ double value() const { return unord_f64(hi); }
    __device__ __forceinline__ int32_t key() const { return (int32_t)~lo; }
};
template <typename V> struct KeyOf;
template <> struct KeyOf<float> { using type = Key64; };
template <> struct KeyOf<double> { using type = Key96; };

template <typename KT>
__device__ __forceinline__ KT wave_max_key(KT b) {
    b.take_max(b.template via_dpp<DPP_XOR1>());
    b.take_max(b.template via_dpp<DPP_XOR2>());
    b.take_max(b.template via_dpp<DPP_HALF_MIRROR>());
    b.take_max(b.template via_dpp<DPP_MIRROR>());
    b.take_max(b.via_xor(16));
    b.take_max(b.via_xor(32));
    return b;
}

// `rounds` extractions from the R register candidates of each lane of ONE wave; lane 0 records
// them.  Exhausted slots come out as (-inf, KEY_NONE).
template <typename V, int R>
__device__ __forceinline__ void wave_rounds(V (&v)[R], int32_t (&key)[R], int rounds, V *out_v, int32_t *out_k,
                                            int lane) {
    using KT = typename KeyOf<V>::type;
    KT c[R];
#pragma unroll
    for (int j = 0; j < R; ++j) c[j] = key[j] == KEY_NONE ? KT::none() : KT::make(v[j], key[j]);
    for (int r = 0; r < rounds; ++r) {
        KT b = c[0];
#pragma unroll
        for (int j = 1; j < R; ++j) b.take_max(c[j]);
        b = wave_max_key(b);
        if (lane == 0) {
            out_v[r] = b.empty() ? (V)-INFINITY : b.value();
            out_k[r] = b.empty() ? KEY_NONE : b.key();
        }
#pragma unroll
        for (int j = 0; j < R; ++j) c[j] = c[j].same(b) ? KT::none() : c[j];
    }
}

template <typename V, int R, typename F>
__device__ __forceinline__ void wave_select_single(int n, int rounds, F get, V *out_v, int32_t *out_k) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        V v[R];
        int32_t key[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int i = tid + j * 64;
            V tv; int32_t tk;
            const bool ok = get(min(i, n - 1), tv, tk) && i < n && tv == tv;     // see wg_select: loads never sit behind a branch
            v[j] = ok ? tv : (V)-INFINITY; key[j] = ok ? tk : KEY_NONE;
        }
        wave_rounds<V, R>(v, key, rounds, out_v, out_k, tid);
    }
    __syncthreads();
}

// Order-preserving unsigned image of a candidate value (the high part of Key64 / Key96)
template <typename V> struct OrdOf;
template <> struct OrdOf<float> {
    using H = uint32_t;
    static constexpr int BITS = 32;
    __device__ __forceinline__ static H ord(float v) { return ord_f32(v); }
    __device__ __forceinline__ static H lane_value(H v, int l) { return (H)__builtin_amdgcn_readlane((int)v, l); }
    // lanes with v >= c as a wave mask (v_cmp straight into an SGPR pair; __ballot(v >= c) compiles to a select + re-compare)
    __device__ __forceinline__ static uint64_t lanes_ge(H v, H c) { return __builtin_amdgcn_uicmp(v, c, 35 /* ICMP_UGE */); }
};
template <> struct OrdOf<double> {
    using H = uint64_t;
    static constexpr int BITS = 64;
    __device__ __forceinline__ static H ord(double v) { return ord_f64(v); }
    __device__ __forceinline__ static H lane_value(H v, int l) {
        return ((H)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, l);
    }
    __device__ __forceinline__ static uint64_t lanes_ge(H v, H c) { return __builtin_amdgcn_uicmpl(v, c, 35 /* ICMP_UGE */); }
};

// The same selection as wave_select_single (one wave holds all n <= 64*R candidates; same results, slot for slot) without
// its `rounds` serial max-extractions (each a 64-lane reduction of 64/96-bit keys):
//   1. pivot: every lane takes the largest value it holds; the rounds-th largest of those 64 lane maxima (found by
//      counting, v_readlane broadcasts) is a lower bound P of the rounds-th largest candidate overall;
//   2. the candidates >= P -- at least `rounds`, for scattered data a few more -- are compacted into an LDS list;
//   3. every list entry computes its rank by counting the entries that sort before it and the first `rounds` ranks are
//      written out.  Sort key = (ord(value), ~key) as in Key64 / Key96 (keys are unique).
// More than 64 candidates >= P (the large values crowd into few lanes, or fewer than `rounds` lanes hold anything): a
// bitwise binary search finds the exact rounds-th largest key instead (v_cmp + s_bcnt1 per register and bit; as slow as
// the serial extraction, but rare).  In-kernel stamps, 17 rounds over 992 candidates: serial extraction ~9 us, binary
// search 6.9 + 2.5 us, pivot ~2.5 us.  Needs rounds <= 64.
template <typename V, int R, typename F>
__device__ __forceinline__ void wave_select_thresh(int n, int rounds, F get, V *out_v, int32_t *out_k) {
    using O = OrdOf<V>;
    using H = typename O::H;
    __shared__ V cv[64];
    __shared__ int32_t ck[64];
    const int tid = threadIdx.x;
    if (tid < 64) {
        H hi[R];
        uint32_t lo[R];        // ~key; 0 = empty slot (real keys are < KEY_NONE, so their ~key has the top bit set)
        V val[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int i = tid + j * 64;
            V tv; int32_t tk;
            const bool ok = get(min(i, n - 1), tv, tk) && i < n && tv == tv;     // see wg_select: loads never sit behind a branch
            hi[j] = ok ? O::ord(tv) : 0; lo[j] = ok ? ~(uint32_t)tk : 0; val[j] = ok ? tv : (V)-INFINITY;
        }
        // Empty slots have hi == 0; no real value maps to 0 (ord() of a non-NaN is >= 0x007fffff).
        auto count_ge = [&](H c) {
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < R; ++j) cnt += __popcll(O::lanes_ge(hi[j], c));
            return cnt;
        };
        // 1. pivot
        H lm = hi[0];
#pragma unroll
        for (int j = 1; j < R; ++j) lm = hi[j] > lm ? hi[j] : lm;
        int lrank = 0;                      // lane maxima ranked (ties: lower lane first): a permutation of 0..63
        for (int l = 0; l < 64; ++l) {
            const H o = O::lane_value(lm, l);
            lrank += (o > lm || (o == lm && l < tid)) ? 1 : 0;
        }
        const int pl = __ffsll((long long)__ballot(lrank == rounds - 1)) - 1;
        H P = O::lane_value(lm, pl);
        P = P ? P : 1;                      // fewer than `rounds` lanes hold anything: every candidate is at or above the pivot
        // exact cut, only when the pivot lets too many through
        bool exact = false;
        H T = 0;
        uint32_t TL = 0;
        if (count_ge(P) > 64) {
            exact = true;
            // T = the rounds-th largest high part (0 when fewer than `rounds` candidates exist: then all of them are taken)
            for (int bit = O::BITS - 1; bit >= 0; --bit) {
                const H c = T | ((H)1 << bit);
                if (count_ge(c) >= rounds) T = c;
            }
            // equal values straddling the cut: among hi == T keep the `need` largest low parts (= smallest keys)
            auto count = [&](auto pred) {
                int c = 0;
#pragma unroll
                for (int j = 0; j < R; ++j) c += __popcll(__ballot(pred(j)));
                return c;
            };
            if (count([&](int j) { return hi[j] != 0 && hi[j] >= T; }) > rounds) {
                const int need = rounds - count([&](int j) { return hi[j] != 0 && hi[j] > T; });
                for (int bit = 31; bit >= 0; --bit) {
                    const uint32_t c = TL | (1u << bit);
                    if (count([&](int j) { return hi[j] == T && lo[j] >= c; }) >= need) TL = c;
                }
            }
        }
        // 2. compact the survivors (at most 64) into the list, in any order
        int m = 0;
        const uint64_t below = ((uint64_t)1 << tid) - 1;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const bool take = exact ? (hi[j] != 0 && (hi[j] > T || (hi[j] == T && lo[j] >= TL))) : hi[j] >= P;
            const uint64_t mask = __ballot(take);
            if (take) {
                const int slot = m + __popcll(mask & below);
                cv[slot] = val[j];
                ck[slot] = (int32_t)~lo[j];
            }
            m += __popcll(mask);
        }
        // 3. one survivor per lane; its rank = number of survivors that sort before it.  (LDS executes a wave's accesses
        // in order; the clobber only keeps the compiler from moving the cross-lane reads above the writes.)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        V mv = (V)-INFINITY;
        int32_t mk = KEY_NONE;
        if (tid < m) { mv = cv[tid]; mk = ck[tid]; }
        const H mh = tid < m ? O::ord(mv) : 0;
        const uint32_t ml = tid < m ? ~(uint32_t)mk : 0;
        int rank = 0;
        for (int i = 0; i < m; ++i) {
            const H bh = O::lane_value(mh, i);
            const uint32_t bl = (uint32_t)__builtin_amdgcn_readlane((int)ml, i);
            rank += (bh > mh || (bh == mh && bl > ml)) ? 1 : 0;
        }
        if (tid < m && rank < rounds) { out_v[rank] = mv; out_k[rank] = mk; }
        if (tid >= m && tid < rounds) { out_v[tid] = (V)-INFINITY; out_k[tid] = KEY_NONE; }
    }
    __syncthreads();
}

template <typename V, int R, typename F>
__device__ __forceinline__ void wg_select_regs(int n, int rounds, F get, V *out_v, int32_t *out_k, SelScratch<V> *sc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = FIN_THREADS / 64;
    V v[R];
    int32_t key[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = tid + j * FIN_THREADS;
        V tv; int32_t tk;
        const bool ok = get(min(i, n - 1), tv, tk) && i < n && tv == tv;         // see wg_select: loads never sit behind a branch
        v[j] = ok ? tv : (V)-INFINITY; key[j] = ok ? tk : KEY_NONE;
    }
    wave_rounds<V, R>(v, key, rounds, sc->pv[wave], sc->pk[wave], lane);
    __syncthreads();
    if (wave == 0) {
        constexpr int R2 = (NW * (K_MAX + 1) + 63) / 64;
        V v2[R2];
        int32_t k2[R2];
#pragma unroll
        for (int j = 0; j < R2; ++j) {
            const int cnd = lane + j * 64;
            const bool ok = cnd < NW * rounds;
            const int p = ok ? cnd / rounds : 0, rr = ok ? cnd % rounds : 0;
            v2[j] = ok ? sc->pv[p][rr] : (V)-INFINITY;
            k2[j] = ok ? sc->pk[p][rr] : KEY_NONE;
        }
        wave_rounds<V, R2>(v2, k2, rounds, out_v, out_k, lane);
    }
    __syncthreads();
}

// Workgroup selection over n >= 1 candidates.  get(i, v, key) -> bool valid; keys unique, < KEY_NONE.
// get() is called for every register slot with an index clamped into [0, n) and must be BRANCH-FREE (select its
// addresses, load unconditionally, return the validity): a load behind a divergent branch makes hipcc wait for it before
// the next slot's branch, i.e. one exposed memory latency per register slot -- 16 x ~1.1 us in select_kernel's second level
// (measured with in-kernel stamps: 20 of the kernel's 29 us).
// n <= 4096: candidates live in registers, each wave extracts its own `rounds` winners, wave 0
// merges the 4 lists (2 barriers in all).  Larger n: one global sweep per round (slow, rare).
// Results land in out_v/out_k (shared memory) and are visible to every thread on return.
template <typename V, typename F>
__device__ void wg_select(int n, int rounds, F get, V *out_v, int32_t *out_k, SelScratch<V> *sc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = FIN_THREADS / 64;
    if (n <= 64 * SEL_R) {
        // n <= 1024 (the usual case): one wave holds every candidate, no merge stage, one barrier
        // more than a few rounds: pivot + rank-by-counting instead of serial extraction (same results)
        const bool thresh = MMR_SEL_THRESH && rounds <= 64 && rounds >= 6;
        if (n <= 64 * 8) {
            if (thresh) wave_select_thresh<V, 8>(n, rounds, get, out_v, out_k);
            else wave_select_single<V, 8>(n, rounds, get, out_v, out_k);
        } else {
            if (thresh) wave_select_thresh<V, SEL_R>(n, rounds, get, out_v, out_k);
            else wave_select_single<V, SEL_R>(n, rounds, get, out_v, out_k);
        }
        return;
    }
    if (n <= SEL_FAST_MAX) {
        wg_select_regs<V, SEL_R>(n, rounds, get, out_v, out_k, sc);
        return;
    }
    V pv = (V)INFINITY;
    int32_t pk = -1;
    for (int r = 0; r < rounds; ++r) {
        V bv = (V)-INFINITY;
        int32_t bk = KEY_NONE;
        for (int i = tid; i < n; i += FIN_THREADS) {
            V x; int32_t kx;
            if (!get(i, x, kx) || !(x == x)) continue;
            if (r > 0 && !before(pv, pk, x, kx)) continue;  // taken in an earlier round
            if (before(x, kx, bv, bk)) { bv = x; bk = kx; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const V ov = __shfl_xor(bv, off, 64);
            const int32_t ok = __shfl_xor(bk, off, 64);
            if (before(ov, ok, bv, bk)) { bv = ov; bk = ok; }
        }
        if (lane == 0) { sc->pv[wave][0] = bv; sc->pk[wave][0] = bk; }
        __syncthreads();
        if (tid == 0) {
            V fv = sc->pv[0][0];
            int32_t fk = sc->pk[0][0];
            for (int w = 1; w < NW; ++w)
                if (before(sc->pv[w][0], sc->pk[w][0], fv, fk)) { fv = sc->pv[w][0]; fk = sc->pk[w][0]; }
            sc->bv = fv; sc->bk = fk;
            out_v[r] = fv; out_k[r] = fk;
        }
        __syncthreads();
        pv = sc->bv; pk = sc->bk;
        if (pk == KEY_NONE) {  // exhausted: the remaining slots are empty
            if (tid == 0) for (int rr = r + 1; rr < rounds; ++rr) { out_v[rr] = (V)-INFINITY; out_k[rr] = KEY_NONE; }
            __syncthreads();
            return;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// finalize, in three launches so the exact re-score runs wide instead of inside one workgroup:
//   select_kernel   grid Q        picks the KS best tasks, then the KS best tiles inside them
//   rescore_kernel  grid (KS, Q)  exact fp64 dots of the 32 rows of one candidate tile
//   rank_kernel     grid Q        (-dot64, +row) top-k of the KS*32 candidates + the certificate
// ---------------------------------------------------------------------------------------------
// per query: best excluded approx max, ||q||_2, and whether any tile was left out at all (a bound of -inf alone cannot
// tell "nothing excluded" from "an excluded tile whose live rows all score -inf or NaN")
struct FinMeta { float bound; float qnorm; int32_t excluded; };

__global__ __launch_bounds__(FIN_THREADS) void select_kernel(
    int ks, int ntiles, int tpt, int ntasks, int qpad, const float *__restrict__ bmax,
    const float *__restrict__ tmax, int32_t *__restrict__ sel_tiles /*[Q][KS_MAX]*/, FinMeta *__restrict__ meta,
    const int32_t *__restrict__ gate)
{
    __shared__ SelScratch<float> scf;
    __shared__ float sel_v[KS_MAX + 1];
    __shared__ int32_t sel_task[KS_MAX + 1];
    __shared__ int32_t sel_tile[KS_MAX + 1];
    const int qi = blockIdx.x, tid = threadIdx.x;
    if (gate && gate[qi] == 0) return;          // second tier of the fp32 search: only queries the first tier left open

    // level 1: best ks tasks (+1 to learn the best excluded one)
    wg_select<float>(ntasks, ks + 1, [&](int i, float &v, int32_t &key) {
        v = tmax[(size_t)i * qpad + qi]; key = i; return true; }, sel_v, sel_task, &scf);
    const float bound1 = sel_v[ks];  // -inf when no task was left out
    const bool task_left_out = sel_task[ks] != KEY_NONE;
    __syncthreads();
    // level 2: best ks tiles among the selected tasks' tiles, ordered by (-max, +tile)
    // candidate i = (selected task i / 64, tile i % 64 of it): tasks hold at most MAX_TPT = 64 tiles, so the index splits
    // with a shift instead of a division by the run-time tile count (16 divisions per lane were ~1 us of this kernel)
    static_assert(MAX_TPT == 64, "candidate index layout");
    wg_select<float>(ks * MAX_TPT, ks + 1, [&](int i, float &v, int32_t &key) {
        const int slot = i >> 6, t = i & 63;
        const int32_t task = sel_task[slot];
        const int32_t tile = (task == KEY_NONE ? 0 : task) * tpt + t;
        const bool ok = task != KEY_NONE && t < tpt && tile < ntiles;
        v = bmax[(size_t)(ok ? tile : 0) * qpad + qi]; key = tile; return ok; }, sel_v, sel_tile, &scf);
    if (tid < ks) sel_tiles[(size_t)qi * KS_MAX + tid] = sel_tile[tid];
    if (tid == 0) {
        meta[qi].bound = fmaxf(bound1, sel_v[ks]);
        meta[qi].excluded = task_left_out || sel_tile[ks] != KEY_NONE;
    }
}

// bit r of a row mask (scan_pipeline.h); r < N
__device__ __forceinline__ bool row_bit(const uint32_t *__restrict__ row_mask, int64_t r)
{
    return (row_mask[r >> 5] >> (r & 31)) & 1u;
}

// MASKED: a masked row is treated like a row past N
template <typename T, int PER, bool MASKED>
__global__ __launch_bounds__(FIN_THREADS) void rescore_kernel(
    const T *__restrict__ q, const T *__restrict__ gal, int64_t N, int tile_rows,
    const int32_t *__restrict__ sel_tiles, double *__restrict__ cand /*[Q][KS_MAX*32]*/, FinMeta *__restrict__ meta,
    const int32_t *__restrict__ gate, const uint32_t *__restrict__ row_mask)
{
    constexpr int E = PER * 64;
    const int slot = blockIdx.x, qi = blockIdx.y;
    if (gate && gate[qi] == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, grp = tid >> 4;   // 16 row groups
    const int32_t tile = sel_tiles[(size_t)qi * KS_MAX + slot];
    QuadQuery<T, PER> qq;
    qq.load(q + (size_t)qi * E, m);
    QuadRow<T, PER> gr[2];
    bool live[2];
    const int passes = tile_rows / 16;      // 2 for 32-row (bf16) tiles, 1 for 16-row (fp32) tiles
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t row = (int64_t)tile * tile_rows + u * 16 + grp;
        live[u] = u < passes && tile != KEY_NONE && row < N;
        if constexpr (MASKED) live[u] = live[u] && row_bit(row_mask, live[u] ? row : 0);
        gr[u].load(gal + (size_t)(live[u] ? row : 0) * E, m);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const double s = quad_dot<T, PER>(qq, gr[u]);
        if (m == 0 && u < passes) cand[((size_t)qi * KS_MAX + slot) * TILE_ROWS + u * 16 + grp] = live[u] ? s : -INFINITY;
    }
    if (slot == 0 && grp == 0) {   // ||q||: sizes the certificate's margin
        double qn2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) qn2 += chunk_partial<PER>(qq.v[i], qq.v[i]);
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) qn2 += __shfl_xor(qn2, off, 64);
        // never below 2^-100 for a non-zero query: a norm too small for fp32 is overstated (sound), not rounded towards zero
        if (m == 0) meta[qi].qnorm = qn2 > 0.0 ? fmaxf((float)sqrt(qn2), 0x1p-100f) : (float)sqrt(qn2);
    }
}

// MASKED: a candidate is a row whose mask bit is set -- by its bit, not by its value: with fewer than k live rows the
// masked rows' -inf re-scores must not fill the slots
template <bool MASKED>
__global__ __launch_bounds__(FIN_THREADS) void rank_kernel(
    int64_t N, int k, int ks, int tile_rows, const int32_t *__restrict__ sel_tiles, const double *__restrict__ cand,
    const FinMeta *__restrict__ meta, float scale, float eps_rel, float host_bound,
    const float *__restrict__ dev_bound, int32_t *__restrict__ idx,
    float *__restrict__ score, double *__restrict__ dot64, int32_t *__restrict__ status,
    int32_t *__restrict__ need_exact, const int32_t *__restrict__ gate, const float *__restrict__ qres,
    const float *__restrict__ gres_dev, float gres_rel, const uint32_t *__restrict__ row_mask)
{
    __shared__ SelScratch<double> scd;
    __shared__ double out_v[K_MAX];
    __shared__ int32_t out_k[K_MAX];
    const int qi = blockIdx.x, tid = threadIdx.x;
    if (gate && gate[qi] == 0) return;          // (gate aliases need_exact: this workgroup is its only writer)
    const int32_t *st = sel_tiles + (size_t)qi * KS_MAX;
    const double *cs = cand + (size_t)qi * KS_MAX * TILE_ROWS;
    // candidate i = (slot i / tile_rows, row-in-tile i % tile_rows); cand keeps a 32-entry stride per slot
    const int tr_shift = tile_rows == 32 ? 5 : 4;                     // tile_rows is 32 (bf16) or 16 (fp32)
    wg_select<double>(ks * tile_rows, k, [&](int i, double &v, int32_t &key) {
        const int slot = i >> tr_shift, rr = i & (tile_rows - 1);
        const int32_t tile = st[slot];
        const int64_t row = (int64_t)(tile == KEY_NONE ? 0 : tile) * tile_rows + rr;
        key = (int32_t)row; v = cs[slot * TILE_ROWS + rr];
        if constexpr (MASKED) return tile != KEY_NONE && row < N && row_bit(row_mask, row < N ? row : N - 1);
        return tile != KEY_NONE && row < N; }, out_v, out_k, &scd);
    if (tid < k) {
        const size_t o = (size_t)qi * k + tid;
        const bool has = out_k[tid] != KEY_NONE;
        idx[o] = has ? out_k[tid] : -1;
        score[o] = has ? (float)(out_v[tid] * (double)scale) : -INFINITY;
        if (dot64) dot64[o] = has ? out_v[tid] : -INFINITY;
    }
    if (tid == 0) {
        // Certificate: every excluded tile's max (an fp32 MFMA dot) is <= bound; a row of an excluded
        // tile can only displace the k-th pick if its exact dot reaches kth, i.e. if bound + err >= kth.
        // margin = eps_rel * ||q|| * (largest gallery row norm): the caller's bound and/or the one measured on the
        // device (mmr_gallery_norm_bound); when both are given the larger one wins, so an understated caller bound
        // cannot shrink the margin below what the data needs
        const double bound = (double)meta[qi].bound;
        float gnorm = host_bound;
        if (dev_bound) gnorm = fmaxf(gnorm, *dev_bound);
        // + an absolute term for sums in the fp32 subnormal range, where roundings are absolute (to the 2^-149 grid) and a
        // relative margin does not cover them: at most 3 * 1024 products and as many adds, each off by <= 2^-150 (MFMA
        // accumulators keep subnormals) -- 3 * 1024 * 2 * 2^-150 < 2^-137
        double eps = (double)eps_rel * (double)gnorm * (double)meta[qi].qnorm + 0x1p-137;
        if (qres) {
            // first tier of the split fp32 search: the scan multiplied bf16(q) with hi(g).
            // |q.g - qh.gh| <= |q - qh| |g| + |qh| |g - gh|, with |q - qh| measured per query, |g - gh| <= the measured maximum
            // over the gallery's rows (or gres_rel * the norm bound when the caller has none) and |qh| <= (1 + 2^-8) |q|
            const double gres = gres_dev ? (double)*gres_dev : (double)gres_rel * (double)gnorm;
            eps += (double)qres[qi] * (double)gnorm + (double)meta[qi].qnorm * (1.0 + 0x1p-8) * gres;
        }
        const int kk = (int)(N < k ? N : k);
        // No tile left out: every row was re-scored exactly, nothing to certify.  Otherwise the list must be full and its
        // k-th value must clear bound + eps; a short list next to excluded tiles is never certified, because a row whose dot
        // is -inf (it fills a slot when fewer than k better rows exist) hides in a tile whose maximum is -inf like a dead
        // tile's.  NaN or infinite eps (a NaN query, an infinite norm bound, 0 * inf) fails the comparison: exhaustive path.
        // The fp32 accumulations of the scan cannot overflow while |q| * G < FLT_MAX (every partial sum is at most
        // sum |q_i g_i| <= |q||g|); beyond that a tile maximum may be NaN (inf - inf) and silently skipped, so such a query is
        // not certified either.  1.01: the split scans' operands are up to 1 + 2^-8 longer than the rows.
        const bool overflow_safe = (double)gnorm * (double)meta[qi].qnorm * 1.01 < (double)__FLT_MAX__;
        const bool ok = !meta[qi].excluded ||
                        (overflow_safe && out_k[kk - 1] != KEY_NONE && out_v[kk - 1] > bound + eps);
        need_exact[qi] = ok ? 0 : 1;
        if (status) status[qi] = ok ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------------
// exhaustive exact path
// ---------------------------------------------------------------------------------------------
struct ExhEntry { double s; int32_t i; int32_t pad; };

// Insert a wave-uniform (s, id) into the lane-distributed sorted list (lane j = j-th best).
__device__ __forceinline__ void list_insert(double &my_s, int32_t &my_i, double s, int32_t id, int lane) {
    const bool before_me = before(s, id, my_s, my_i);
    const double ps = __shfl_up(my_s, 1, 64);
    const int32_t pi = __shfl_up(my_i, 1, 64);
    if (before_me) {
        const bool before_prev = lane > 0 && before(s, id, ps, pi);
        my_s = before_prev ? ps : s;
        my_i = before_prev ? pi : id;
    }
}

// MASKED: masked rows are skipped
template <typename T, int PER, bool MASKED>
__global__ __launch_bounds__(256) void exh_scan_kernel(
    const T *__restrict__ q, const T *__restrict__ gal, int64_t N, int K, int nslab, int64_t rows_per_slab,
    const int32_t *__restrict__ need_exact, ExhEntry *__restrict__ partial, const uint32_t *__restrict__ row_mask)
{
    constexpr int E = PER * 64;
    __shared__ ExhEntry lists[4][K_MAX];
    const int qi = blockIdx.y, slab = blockIdx.x;
    if (need_exact && need_exact[qi] == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, sub = lane >> 4;

    QuadQuery<T, PER> qq;
    qq.load(q + (size_t)qi * E, m);

    double my_s = -INFINITY;
    int32_t my_i = KEY_NONE;
    const int64_t r0 = (int64_t)slab * rows_per_slab;
    const int64_t r1 = min(N, r0 + rows_per_slab);
    // each wave pass covers 4 consecutive rows (one per 16-lane group); waves interleave by 4 rows
    for (int64_t rb = r0 + wave * 4; rb < r1; rb += 16) {
        const int64_t r = rb + sub;
        const bool live = r < r1;
        QuadRow<T, PER> gr;
        gr.load(gal + (size_t)(live ? r : rb) * E, m);
        const double s = quad_dot<T, PER>(qq, gr);
        bool rlive = live;
        if constexpr (MASKED) rlive = live && row_bit(row_mask, live ? r : rb);
        const uint64_t lmask = __ballot(rlive);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double sg = __shfl(s, 16 * g, 64);
            const int64_t rg = rb + g;
            if ((MASKED ? ((lmask >> (16 * g)) & 1) : rg < r1) && sg == sg) {
                const double ts = __shfl(my_s, K - 1, 64);
                const int32_t ti = __shfl(my_i, K - 1, 64);
                if (before(sg, (int32_t)rg, ts, ti)) list_insert(my_s, my_i, sg, (int32_t)rg, lane);
            }
        }
    }
    lists[wave][lane] = ExhEntry{my_s, my_i, 0};
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < 4; ++w)
            for (int j = 0; j < K; ++j) {
                const ExhEntry e = lists[w][j];
                if (e.i == KEY_NONE) break;
                const double ts = __shfl(my_s, K - 1, 64);
                const int32_t ti = __shfl(my_i, K - 1, 64);
                if (before(e.s, e.i, ts, ti)) list_insert(my_s, my_i, e.s, e.i, lane);
            }
        if (lane < K) partial[((size_t)qi * nslab + slab) * K + lane] = ExhEntry{my_s, my_i, 0};
    }
}

__global__ __launch_bounds__(FIN_THREADS) void exh_merge_kernel(
    const ExhEntry *__restrict__ partial, int K, int k, int nslab, float scale,
    const int32_t *__restrict__ need_exact, int32_t *__restrict__ idx, float *__restrict__ score,
    double *__restrict__ dot64)
{
    __shared__ SelScratch<double> sc;
    __shared__ double out_v[K_MAX];
    __shared__ int32_t out_k[K_MAX];
    const int qi = blockIdx.x;
    if (need_exact && need_exact[qi] == 0) return;
    const ExhEntry *p = partial + (size_t)qi * nslab * K;
    wg_select<double>(nslab * K, k, [&](int i, double &v, int32_t &key) {
        const ExhEntry e = p[i];
        v = e.s; key = e.i; return e.i != KEY_NONE; }, out_v, out_k, &sc);
    const int tid = threadIdx.x;
    if (tid < k) {
        const size_t o = (size_t)qi * k + tid;
        const bool has = out_k[tid] != KEY_NONE;
        idx[o] = has ? out_k[tid] : -1;
        score[o] = has ? (float)(out_v[tid] * (double)scale) : -INFINITY;
        if (dot64) dot64[o] = has ? out_v[tid] : -INFINITY;
    }
}

// ---------------------------------------------------------------------------------------------
// small dense ops
// ---------------------------------------------------------------------------------------------
template <typename T, int PER>
__global__ __launch_bounds__(256) void similarity_kernel(const T *__restrict__ q, const T *__restrict__ gal,
                                                          int Q, int64_t N, float scale, float *__restrict__ out)
{
    constexpr int E = PER * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 4 + wave;
    if (n >= N) return;
    float gv[PER];
    load_chunk<T, PER>(gal + (size_t)n * E, lane, gv);
    for (int qi = 0; qi < Q; ++qi) {
        float qv[PER];
        load_chunk<T, PER>(q + (size_t)qi * E, lane, qv);
        const double s = exact_dot<PER>(qv, gv);
        if (lane == 0) out[(size_t)qi * N + n] = (float)(s * (double)scale);
    }
}

// Tip-Adapter logits, fused (reference code/main_custom.py:111,124-127, code/utils.py:182-186):
//   clip_logits  = 100 * F @ W                      F[N,E], W^T given as wt[C,E]
//   affinity     = F @ Kc                           Kc^T given as kt[S,E]
//   cache_logits = exp(-(beta - beta*affinity)) @ V * 10        V[S,C]
//   tip_logits   = clip_logits + alpha * cache_logits
// One wave per feature row: the row stays in registers, every key/class row is a coalesced read,
// the [N,S] affinity matrix is never written.  fp32 accumulate.
template <typename T, int PER>
__global__ __launch_bounds__(256) void tip_logits_kernel(const T *__restrict__ f, const T *__restrict__ wt,
                                                          const T *__restrict__ kt, const float *__restrict__ v,
                                                          int64_t N, int C, int S, float alpha, float beta,
                                                          float *__restrict__ tip, float *__restrict__ clip)
{
    constexpr int E = PER * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 4 + wave;
    if (n >= N) return;
    float fv[PER];
    load_chunk<T, PER>(f + (size_t)n * E, lane, fv);
    float my_clip = 0.f, my_cache = 0.f;      // lane c < C owns class c
    for (int c = 0; c < C; ++c) {
        float xv[PER];
        load_chunk<T, PER>(wt + (size_t)c * E, lane, xv);
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) p += fv[j] * xv[j];
        p = wave_sum(p);
        if (lane == c) my_clip = 100.f * p;
    }
    for (int s = 0; s < S; ++s) {
        float xv[PER];
        load_chunk<T, PER>(kt + (size_t)s * E, lane, xv);
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) p += fv[j] * xv[j];
        p = wave_sum(p);
        const float e = __expf(-(beta - beta * p));
        if (lane < C) my_cache += e * v[(size_t)s * C + lane];
    }
    if (lane < C) {
        tip[(size_t)n * C + lane] = my_clip + alpha * (my_cache * 10.f);
        if (clip) clip[(size_t)n * C + lane] = my_clip;
    }
}

// element j of a row as fp32, by element type (bf16_t is raw bits; f16_t and float convert)
template <typename T>
__device__ __forceinline__ float row_elem(const T *p, int j)
{
    if constexpr (__is_same(T, bf16_t)) return bf16_to_f32(p[j]);
    else return (float)p[j];
}

template <typename T>
__global__ __launch_bounds__(256) void l2norm_kernel(T *__restrict__ x, int64_t rows, int E)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    if (r >= rows) return;
    T *p = x + (size_t)r * E;
    float ss = 0.f;
    for (int j = lane; j < E; j += 64) {
        const float v = row_elem(p, j);
        ss += v * v;
    }
    ss = wave_sum(ss);
    const float inv = 1.0f / sqrtf(ss);
    for (int j = lane; j < E; j += 64) {
        if constexpr (__is_same(T, bf16_t)) p[j] = f32_to_bf16(row_elem(p, j) * inv);
        else p[j] = (T)(row_elem(p, j) * inv);       // fp16: round-to-nearest-even, like the bf16 store
    }
}

// Largest row L2 norm of a gallery: sizes the certificate's margin (rank_kernel) from the data instead of from a
// caller's promise.  One wave per row, 16-byte loads, grid-stride; each wave keeps its maximum of sum(x^2) and
// lane 0 publishes sqrt(max) with one integer atomicMax (non-negative floats order like their bit patterns).
// The sum of squares is accumulated in fp64 (exact products), so the bound holds at every scale of the rows.  One pass.
template <typename T>
__global__ __launch_bounds__(256) void rownorm_max_kernel(const T *__restrict__ gal, int64_t N, int E,
                                                           unsigned int *__restrict__ out_bits)
{
    constexpr int VEC = 16 / sizeof(T);        // elements per 16-byte load
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = E / VEC;
    double mx = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < N; r += (int64_t)gridDim.x * 4) {
        const T *p = gal + (size_t)r * E;
        double ss = 0.0;                       // fp64: exact squares at any scale (fp32 squares underflow below |x| ~ 2^-63)
        for (int c = lane; c < chunks; c += 64) {
            if constexpr (__is_same(T, bf16_t)) {
                const bf16x8 x = *reinterpret_cast<const bf16x8 *>(p + c * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const double v = bf16_to_f32((bf16_t)x[j]); ss += v * v; }
            } else if constexpr (__is_same(T, f16_t)) {
                const f16x8 x = *reinterpret_cast<const f16x8 *>(p + c * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) { const double v = (float)x[j]; ss += v * v; }
            } else {
                const float4 x = *reinterpret_cast<const float4 *>(p + c * 4);
                ss += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
            }
        }
        ss = wave_sum_f64_butterfly(ss);
        mx = fmax(mx, ss);                     // NaN rows are skipped here like they are by the ranking
    }
    // +inf for a row with an Inf, or whose sum of squares is past FLT_MAX (norm_upper_f32)
    if (lane == 0) atomicMax(out_bits, __float_as_uint(norm_upper_f32(mx, 1.000001f)));
}

// Largest row norm of (gallery - hi): the gallery half of the first-tier margin of the split fp32 search.  Same shape as
// rownorm_max_kernel; the differences are exact fp32 values (residuals of a rounding).
__global__ __launch_bounds__(256) void split_resid_max_kernel(const float *__restrict__ gal, const bf16_t *__restrict__ hi, int64_t N,
                                                              int E, unsigned int *__restrict__ out_bits)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < N; r += (int64_t)gridDim.x * 4) {
        const float *p = gal + (size_t)r * E;
        const bf16_t *ph = hi + (size_t)r * E;
        double ss = 0.0;
        for (int c = lane; c < E / 8; c += 64) {
            const float4 a0 = *reinterpret_cast<const float4 *>(p + c * 8), a1 = *reinterpret_cast<const float4 *>(p + c * 8 + 4);
            const bf16x8 h = *reinterpret_cast<const bf16x8 *>(ph + c * 8);
            const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double d = x[j] - bf16_to_f32((bf16_t)h[j]); ss += d * d; }
        }
        ss = wave_sum_f64_butterfly(ss);
        mx = fmax(mx, ss);                     // (an Inf element's residual inf - inf is NaN: skipped; its row makes the norm bound +inf)
    }
    if (lane == 0) atomicMax(out_bits, __float_as_uint(norm_upper_f32(mx, 1.00001f)));
}

// out[w] = bits (keep[32w + b] != 0) & (and_mask ? and_mask[w] : ~0): one row per thread, one ballot per 64 rows.  Rows at
// or past N read as 0, so the last word's bits past N are clear.
__global__ __launch_bounds__(256) void row_mask_pack_kernel(const uint8_t *__restrict__ keep, const uint32_t *__restrict__ and_mask,
                                                            int64_t N, uint32_t *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint64_t bits = __ballot(r < N && keep[r < N ? r : 0] != 0);
    const int64_t w = r >> 5;
    if ((lane & 31) == 0 && w < ((N + 31) >> 5)) {
        uint32_t v = (uint32_t)(bits >> (lane & 32));
        if (and_mask) v &= and_mask[w];
        out[w] = v;
    }
}

__global__ void fill_empty_kernel(int32_t *idx, float *score, double *dot64, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        idx[i] = -1;
        score[i] = -INFINITY;
        if (dot64) dot64[i] = -INFINITY;
    }
}

// this rank's message for the all-gather: packed[q][j] = (global id = local id + offset, or -1; fp64 dot bits)
__global__ void pack_kernel(const int32_t *__restrict__ idx, const double *__restrict__ dot, int64_t offset, int n,
                            int64_t *__restrict__ packed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int32_t li = idx[i];
        packed[2 * (size_t)i] = li >= 0 ? (int64_t)li + offset : -1;
        packed[2 * (size_t)i + 1] = __double_as_longlong(dot[i]);
    }
}

// parts*k <= 8*64 candidates with int64 global ids: one wave, candidates in registers.
// PACKED: the lists arrive as the gathered messages themselves, [parts][Q][k][2] int64 = (id, dot bits).
template <bool PACKED>
__global__ __launch_bounds__(64) void merge_kernel(const int64_t *__restrict__ idx_parts,
                                                    const double *__restrict__ dot_parts, int parts, int Q, int k,
                                                    float scale, int64_t *__restrict__ idx, float *__restrict__ score,
                                                    double *__restrict__ dot64)
{
    constexpr int R = 16;  // 64 lanes * 16 = 1024 candidates >= MERGE_MAX_PARTS * K_MAX
    const int qi = blockIdx.x, lane = threadIdx.x;
    const int n = parts * k;
    double v[R];
    int64_t key[R];
    constexpr int64_t NONE = 0x7fffffffffffffffLL;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = lane + j * 64;
        v[j] = -INFINITY; key[j] = NONE;
        if (i < n) {
            const size_t o = ((size_t)(i / k) * Q + qi) * k + (i % k);
            const int64_t gi = PACKED ? idx_parts[2 * o] : idx_parts[o];
            const double d = PACKED ? __longlong_as_double(idx_parts[2 * o + 1]) : dot_parts[o];
            if (gi >= 0 && d == d) { v[j] = d; key[j] = gi; }
        }
    }
    for (int r = 0; r < k; ++r) {
        double bv = v[0];
        int64_t bk = key[0];
#pragma unroll
        for (int j = 1; j < R; ++j)
            if (before(v[j], key[j], bv, bk)) { bv = v[j]; bk = key[j]; }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int64_t ok = __shfl_xor(bk, off, 64);
            if (before(ov, ok, bv, bk)) { bv = ov; bk = ok; }
        }
        if (lane == 0) {
            const size_t o = (size_t)qi * k + r;
            const bool has = bk != NONE;
            idx[o] = has ? bk : -1;
            score[o] = has ? (float)(bv * (double)scale) : -INFINITY;
            if (dot64) dot64[o] = has ? bv : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (key[j] == bk) { v[j] = -INFINITY; key[j] = NONE; }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct SearchPlan : TopkScanGeom {
    int nslab, ks;
    int64_t rows_per_slab;
    bool fast;  // MFMA scan usable
    size_t off_bmax, off_tmax, off_flags, off_partial, off_seltiles, off_cand, off_meta, off_nb, off_qb, off_qres, total;
};

static bool exact_supports_E(int E) { return E == 128 || E == 256 || E == 512 || E == 768 || E == 1024; }

static SearchPlan make_plan(int64_t N, int E, int Q, int k, mmr_dtype dt)
{
    SearchPlan p{};
    p.tile_rows = dt == MMR_F32 ? TILE_ROWS_F32 : TILE_ROWS;
    p.qmax = scan_qmax(E, dt);
    p.ntiles = (int)((N + p.tile_rows - 1) / p.tile_rows);
    ScanTasks t = scan_tasks(p.ntiles);
    // test hook: force the tiles-per-task count (1..64) to reach the large-task-count selection paths
    // with a small gallery
    static const int force_tpt = getenv("MMR_SEARCH_TPT") ? atoi(getenv("MMR_SEARCH_TPT")) : 0;
    if (force_tpt >= 1 && force_tpt <= MAX_TPT) t = scan_tasks_of(p.ntiles, force_tpt);
    p.tpt = t.tpt;
    p.ntasks = t.ntasks;
    p.ks = k + 6 > KS_MAX ? KS_MAX : k + 6;
    p.fast = scan_supports_E(E) && k + 6 <= KS_MAX && N > 0;
    // exhaustive path: 64 row slabs per query when it is THE path; 16 when it only backs up the fast path
    // (it is launched unconditionally there and unflagged queries exit at once: fewer idle workgroups)
    int nslab = (int)((N + 2047) / 2048);
    const int slab_cap = p.fast ? 16 : 64;
    p.nslab = nslab < 1 ? 1 : (nslab > slab_cap ? slab_cap : nslab);
    p.rows_per_slab = (N + p.nslab - 1) / p.nslab;
    const int qc = Q < p.qmax ? (Q + 31) / 32 * 32 : p.qmax;
    const size_t Q1 = Q > 0 ? Q : 1;
    WsLayout l;
    // regions sized by Q and E alone come first: the tiered fp32 search runs a bf16-plan pass and an fp32-plan pass over one
    // workspace, and both must find the flags, the bf16 copy of the queries and the measured norm bound at the same place
    // (the bound is measured once, before the first tier, and read by both)
    p.off_flags = l.take(Q1 * sizeof(int32_t));
    p.off_qb = l.take(Q1 * E * sizeof(bf16_t));
    p.off_qres = l.take(Q1 * sizeof(float));
    p.off_nb = l.take(sizeof(float));       // measured gallery norm bound when the caller gives none
    p.off_bmax = l.take((size_t)p.ntiles * qc * sizeof(float));
    p.off_tmax = l.take((size_t)p.ntasks * qc * sizeof(float));
    p.off_partial = l.take(Q1 * p.nslab * K_MAX * sizeof(ExhEntry));
    p.off_seltiles = l.take((size_t)qc * KS_MAX * sizeof(int32_t));
    p.off_cand = l.take((size_t)qc * KS_MAX * TILE_ROWS * sizeof(double));
    p.off_meta = l.take((size_t)qc * sizeof(FinMeta));
    p.total = l.off;
    return p;
}

// fp32 scan of one query chunk: scan_split_kernel over the caller's hi / lo split (mmr_gallery_split_bf16) when split_hi is
// given, else scan_f32s_kernel over the fp32 rows.  gate: scan_split_kernel's second-tier gate (nullable).
static int launch_scan_f32(int E, const float *qf, const float *gal, const bf16_t *split_hi, const bf16_t *split_lo, int Qc,
                           int64_t N, const TopkScanGeom &g, int qpad, float *bmax, float *tmax, const int32_t *gq,
                           const uint32_t *row_mask, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        return dispatch_masked(row_mask, [&](auto m) -> int {
            constexpr int EE = decltype(e)::value;
            constexpr bool MASKED = decltype(m)::value;
            using C = ScanF32sCfg<EE>;
            if (split_hi)
                return launch_scan_kernel<&scan_split_kernel<EE, MASKED>>(g.ntasks, C::THREADS, C::SPLIT_LDS, st, qf, split_hi,
                                                                          split_lo, Qc, N, g.ntiles, g.tpt, qpad / 16, qpad, bmax,
                                                                          tmax, gq, row_mask);
            return launch_scan_kernel<&scan_f32s_kernel<EE, MASKED>>(g.ntasks, C::THREADS, C::LDS, st, qf, gal, Qc, N, g.ntiles,
                                                                     g.tpt, qpad / 16, qpad, bmax, tmax, row_mask);
        });
    });
}

// The scans above as one call (topk_scan.h): the tiers of mmr_cosine_topk below and pass A of the deep top-k
// (deep_topk.hip), with the tile / task geometry make_plan gives the top-k search.
TopkScanGeom topk_scan_geom(int64_t N, int E, mmr_dtype scan_dtype) { return make_plan(N, E, 1, 1, scan_dtype); }

int launch_topk_scan(mmr_dtype scan_dtype, int E, const void *q, const void *gal, int Qc, int64_t N, const TopkScanGeom &g,
                     int qpad, float *bmax, float *tmax, const uint32_t *row_mask, hipStream_t st, const bf16_t *split_hi,
                     const bf16_t *split_lo, const int32_t *gate)
{
    if (scan_dtype == MMR_BF16) return launch_topk_scan_16(E, (const bf16_t *)q, (const bf16_t *)gal, Qc, N, g, qpad, bmax, tmax, row_mask, st);
    if (scan_dtype == MMR_F16) return launch_topk_scan_16(E, (const f16_t *)q, (const f16_t *)gal, Qc, N, g, qpad, bmax, tmax, row_mask, st);
    return launch_scan_f32(E, (const float *)q, (const float *)gal, split_hi, split_lo, Qc, N, g, qpad, bmax, tmax, gate, row_mask, st);
}

// What the certificate of one tier adds to the margin (rank_kernel): tier 1 of the split search scans bf16-rounded
// queries over the hi half alone; the main tier adds nothing
struct TierMargin {
    const float *qres = nullptr;        // per query ||q - bf16(q)||
    const float *gres_dev = nullptr;    // max_row ||g - hi|| (device scalar, nullable)
    float gres_rel = 0.f;               // ... or this share of the norm bound
};

template <typename T, int PER>
static int launch_finalize(const T *q, const T *gal, int Qc, int64_t N, int k, const SearchPlan &p, int qpad,
                           const float *bmax, const float *tmax, float scale, float eps_rel, const NormBound &nb, int32_t *idx,
                           float *score, double *dot64, int32_t *status, int32_t *flags, int32_t *sel_tiles,
                           double *cand, FinMeta *meta, const uint32_t *row_mask, hipStream_t st, const int32_t *gate,
                           const TierMargin &tm)
{
    ProfScope prof(MMR_PROF_FINALIZE, st);
    hipLaunchKernelGGL(select_kernel, dim3(Qc), dim3(FIN_THREADS), 0, st, p.ks, p.ntiles, p.tpt, p.ntasks, qpad, bmax,
                       tmax, sel_tiles, meta, gate);
    MMR_CHECK_LAUNCH();
    return dispatch_masked(row_mask, [&](auto m) -> int {
        constexpr bool MASKED = decltype(m)::value;
        hipLaunchKernelGGL((rescore_kernel<T, PER, MASKED>), dim3(p.ks, Qc), dim3(FIN_THREADS), 0, st, q, gal, N, p.tile_rows,
                           sel_tiles, cand, meta, gate, row_mask);
        MMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(rank_kernel<MASKED>, dim3(Qc), dim3(FIN_THREADS), 0, st, N, k, p.ks, p.tile_rows, sel_tiles, cand, meta,
                           scale, eps_rel, nb.host, nb.dev, idx, score, dot64, status, flags, gate, tm.qres, tm.gres_dev,
                           tm.gres_rel, row_mask);
        MMR_CHECK_LAUNCH();
        return MMR_OK;
    });
}

template <typename T, int PER>
static int launch_exh(const T *q, const T *gal, int Q, int64_t N, int k, const SearchPlan &p, float scale,
                      const int32_t *flags, ExhEntry *partial, int32_t *idx, float *score, double *dot64,
                      const uint32_t *row_mask, hipStream_t st)
{
    ProfScope prof(MMR_PROF_EXACT, st);
    MMR_TRY(dispatch_masked(row_mask, [&](auto m) -> int {
        hipLaunchKernelGGL((exh_scan_kernel<T, PER, decltype(m)::value>), dim3(p.nslab, Q), dim3(256), 0, st, q, gal, N, k, p.nslab,
                           p.rows_per_slab, flags, partial, row_mask);
        MMR_CHECK_LAUNCH();
        return MMR_OK;
    }));
    hipLaunchKernelGGL(exh_merge_kernel, dim3(Q), dim3(FIN_THREADS), 0, st, partial, k, k, p.nslab, scale, flags, idx,
                       score, dot64);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_norm_bound(const void *gallery, mmr_dtype dtype, int64_t N, int E, float *out, hipStream_t st)
{
    MMR_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float), st));
    if (N == 0) return MMR_OK;
    const dim3 grid(grid_1d(N, 4));
    return dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rownorm_max_kernel<T>, grid, dim3(256), 0, st, (const T *)gallery, N, E, (unsigned int *)out);
        MMR_CHECK_LAUNCH();
        return MMR_OK;
    });
}

// The arguments of one mmr_cosine_topk* call that every tier and the exhaustive path see
struct TopkCall {
    const void *q, *gallery;        // the ORIGINAL rows, `dtype` elements: what the fp64 re-score reads
    mmr_dtype dtype;
    int Q;
    int64_t N;
    int E, k;
    float scale, eps_rel;
    NormBound nb;
    int32_t *idx;
    float *score;
    double *dot64;
    int32_t *status, *flags;
    char *ws;
    const uint32_t *row_mask;
    hipStream_t st;
};

// One tier of the fast path: for each chunk of p.qmax queries, the scan of (scan_q, scan_gal) -- `scan_dtype` elements;
// split_hi / split_lo: the three-product scan -- then select, re-score on the original rows and rank.  gate (nullable):
// per-query flags of the tier before; a query whose flag is clear is skipped.
static int topk_tier(const TopkCall &c, const SearchPlan &p, mmr_dtype scan_dtype, const void *scan_q, const void *scan_gal,
                     const bf16_t *split_hi, const bf16_t *split_lo, const int32_t *gate, const TierMargin &tm)
{
    float *bmax = (float *)(c.ws + p.off_bmax), *tmax = (float *)(c.ws + p.off_tmax);
    const size_t sesz = scan_dtype == MMR_F32 ? 4 : 2;
    for (int q0 = 0; q0 < c.Q; q0 += p.qmax) {
        const int Qc = (c.Q - q0) < p.qmax ? (c.Q - q0) : p.qmax;
        const int qpad = (Qc + 31) / 32 * 32;
        const int32_t *gq = gate ? gate + q0 : nullptr;
        MMR_TRY(launch_topk_scan(scan_dtype, c.E, (const char *)scan_q + (size_t)q0 * c.E * sesz, scan_gal, Qc, c.N, p, qpad, bmax,
                                 tmax, c.row_mask, c.st, split_hi, split_lo, gq));
        TierMargin tq = tm;
        if (tq.qres) tq.qres += q0;
        MMR_TRY(dispatch_elem(c.dtype, [&](auto tag) -> int {
            using T = typename decltype(tag)::type;
            return dispatch_per(c.E, [&](auto per) -> int {
                return launch_finalize<T, decltype(per)::value>(
                    (const T *)c.q + (size_t)q0 * c.E, (const T *)c.gallery, Qc, c.N, c.k, p, qpad, bmax, tmax, c.scale, c.eps_rel,
                    c.nb, c.idx + (size_t)q0 * c.k, c.score + (size_t)q0 * c.k, c.dot64 ? c.dot64 + (size_t)q0 * c.k : nullptr,
                    c.status ? c.status + q0 : nullptr, c.flags + q0, (int32_t *)(c.ws + p.off_seltiles),
                    (double *)(c.ws + p.off_cand), (FinMeta *)(c.ws + p.off_meta), c.row_mask, c.st, gq, tq);
            });
        }));
    }
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_search_workspace_bytes(int64_t N, int E, int Q, int k)
{
    if (N < 0 || Q < 0 || k < 1) return 0;
    const size_t a = make_plan(N, E, Q, k, MMR_BF16).total, b = make_plan(N, E, Q, k, MMR_F32).total;
    return a > b ? a : b;
}

extern "C" int mmr_gallery_norm_bound(const void *gallery, mmr_dtype dtype, int64_t N, int E, float *bound_out, void *stream)
{
    MMR_TRY(EntryCheck{"mmr_gallery_norm_bound"}.dtype(dtype));
    MMR_CHECK_ARG(N >= 0 && E >= 8 && E % 8 == 0, "mmr_gallery_norm_bound: bad shape N=%lld E=%d (E must be a multiple of 8)", (long long)N, E);
    MMR_CHECK_ARG(bound_out && (gallery || N == 0), "mmr_gallery_norm_bound: null pointer");
    MMR_CHECK_ARG(((uintptr_t)gallery & 15) == 0, "mmr_gallery_norm_bound: gallery must be 16-byte aligned");
    return launch_norm_bound(gallery, dtype, N, E, bound_out, (hipStream_t)stream);
}

static int cosine_topk_impl(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                            float scale, float gallery_norm_bound, const float *norm_bound_dev, int32_t *idx, float *score,
                            double *dot64, int32_t *status, void *workspace, size_t workspace_bytes, void *stream,
                            const bf16_t *split_hi = nullptr, const bf16_t *split_lo = nullptr,
                            const float *split_resid_dev = nullptr, const uint32_t *row_mask = nullptr)
{
    const EntryCheck ck{"mmr_cosine_topk"};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.sizes_int32(Q, N));
    MMR_CHECK_ARG(k >= 1 && k <= K_MAX, "mmr_cosine_topk: k=%d outside [1,%d]", k, K_MAX);
    MMR_CHECK_ARG(scale > 0.f, "mmr_cosine_topk: scale must be > 0 (got %g)", (double)scale);
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    if (!exact_supports_E(E)) { set_error("mmr_cosine_topk: E=%d unsupported (128,256,512,768,1024)", E); return MMR_ENOTSUP; }
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(q && idx && score && (gallery || N == 0), "mmr_cosine_topk: null pointer");
    MMR_TRY(ck.aligned16((uintptr_t)q | (uintptr_t)gallery, "q/gallery"));
    MMR_TRY(ck.row_mask(row_mask));
    const SearchPlan p = make_plan(N, E, Q, k, dtype);
    MMR_CHECK_ARG(workspace != nullptr, "mmr_cosine_topk: null workspace");
    MMR_TRY(ck.workspace(workspace_bytes, p.total));
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int32_t *flags = (int32_t *)(ws + p.off_flags);

    if (N == 0) {  // nothing to rank: every slot is empty (idx -1, score -inf)
        hipLaunchKernelGGL(fill_empty_kernel, dim3((Q * k + 255) / 256), dim3(256), 0, st, idx, score, dot64, Q * k);
        MMR_CHECK_LAUNCH();
        if (status) MMR_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)Q * sizeof(int32_t), st));
        return MMR_OK;
    }

    if (p.fast) {
        // fp32 MFMA accumulation error of a length-E dot is <= ~E*2^-24*|q||g| (bf16 x bf16 products are exact
        // in fp32; fp32 x fp32 products add one rounding each, same order); the margin below is that worst case
        // for E<=1024 with headroom.  It gates the fast path only.
        // fp16 operands: products are exact in fp32 like bf16's, and the two f16 MFMA shapes accumulate no worse than the
        // bf16 ones (tools/micro/mfma_acc_probe.hip, DESIGN section 3 "fp16 galleries"), so the margin is the same.
        const float eps_rel = 8e-5f;
        // no bound from the caller: measured here (GalleryIndex-style callers measure once with mmr_gallery_norm_bound and
        // pass the device scalar instead)
        const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, norm_bound_dev, (float *)(ws + p.off_nb), st);
        MMR_TRY(nb.rc);
        const TopkCall c{q, gallery, dtype, Q, N, E, k, scale, eps_rel, nb, idx, score, dot64, status, flags, ws, row_mask, st};
        // MMR_SPLIT_TIERS=0: split galleries go straight to the three-product scan (A/B and tests of that tier alone)
        static const bool tiers = !(getenv("MMR_SPLIT_TIERS") && atoi(getenv("MMR_SPLIT_TIERS")) == 0);
        const bool split = dtype == MMR_F32 && split_hi && split_lo;
        const int32_t *gate = nullptr;
        if (split && tiers) {
            // First tier of the split fp32 search: the bf16 scan over the hi array alone (half the bytes, one MFMA product
            // instead of three) with bf16-rounded queries.  Its scores are off by up to |q - qh||g| + |qh||g - gh| (~1e-3 |q||g|
            // against the three-product scan's 1e-5), so its certificate adds exactly that -- measured per query and over the
            // gallery, see rank_kernel -- to the margin and keeps KS_MAX candidate tiles instead of k + 6; the fp64 re-score
            // reads the fp32 rows as always.  A query it cannot certify keeps its flag and goes through the second tier
            // below -- the three-product scan with the tight margin -- and only then to the exhaustive path.  The second
            // tier's launches return at once when no flag is set.
            SearchPlan p1 = make_plan(N, E, Q, k, MMR_BF16);
            // candidate tiles of this tier; MMR_SPLIT_KS1 = 24 measured the same time on random unit rows and certifies less often
            static const int ks1 = getenv("MMR_SPLIT_KS1") ? atoi(getenv("MMR_SPLIT_KS1")) : KS_MAX;
            if (ks1 > p1.ks && ks1 <= KS_MAX) p1.ks = ks1;
            MMR_TRY(ck.workspace(workspace_bytes, p1.total));
            bf16_t *qb = (bf16_t *)(ws + p1.off_qb);
            float *qres = (float *)(ws + p1.off_qres);
            hipLaunchKernelGGL(queries_to_bf16_kernel, dim3((Q + 3) / 4), dim3(256), 0, st, (const float *)q, Q, E, qb, qres);
            MMR_CHECK_LAUNCH();
            MMR_TRY(topk_tier(c, p1, MMR_BF16, qb, split_hi, nullptr, nullptr, nullptr, TierMargin{qres, split_resid_dev, 0x1p-8f}));
            gate = flags;
        }
        MMR_TRY(topk_tier(c, p, dtype, q, gallery, split ? split_hi : nullptr, split_lo, gate, TierMargin{}));
    } else if (status) {
        // 1 = exhaustive path for every query
        MMR_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)status, 1, (size_t)Q, st));
    }
    // the exhaustive path: the queries the fast path flagged, or, without a fast path, all of them
    return dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return dispatch_per(E, [&](auto per) -> int {
            return launch_exh<T, decltype(per)::value>((const T *)q, (const T *)gallery, Q, N, k, p, scale, p.fast ? flags : nullptr,
                                                       (ExhEntry *)(ws + p.off_partial), idx, score, dot64, row_mask, st);
        });
    });
}

extern "C" int mmr_cosine_topk(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                               float scale, float gallery_norm_bound, int32_t *idx, float *score, double *dot64,
                               int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    return cosine_topk_impl(q, gallery, dtype, Q, N, E, k, scale, gallery_norm_bound, nullptr, idx, score, dot64, status,
                            workspace, workspace_bytes, stream);
}

extern "C" int mmr_cosine_topk_ex(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                                  float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev, int32_t *idx,
                                  float *score, double *dot64, int32_t *status, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    return cosine_topk_impl(q, gallery, dtype, Q, N, E, k, scale, gallery_norm_bound, gallery_norm_bound_dev, idx, score,
                            dot64, status, workspace, workspace_bytes, stream);
}

extern "C" int mmr_cosine_topk_masked(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                                      float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                                      const uint32_t *row_mask, int32_t *idx, float *score, double *dot64, int32_t *status,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    return cosine_topk_impl(q, gallery, dtype, Q, N, E, k, scale, gallery_norm_bound, gallery_norm_bound_dev, idx, score,
                            dot64, status, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, row_mask);
}

extern "C" int mmr_row_mask_pack(const uint8_t *keep, const uint32_t *and_mask, int64_t N, uint32_t *out, void *stream)
{
    MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff, "mmr_row_mask_pack: N=%lld outside [0, 2^31-1)", (long long)N);
    if (N == 0) return MMR_OK;
    MMR_CHECK_ARG(keep && out, "mmr_row_mask_pack: null pointer");
    MMR_CHECK_ARG((((uintptr_t)out | (uintptr_t)and_mask) & 3) == 0, "mmr_row_mask_pack: out / and_mask must be 4-byte aligned");
    hipLaunchKernelGGL(row_mask_pack_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keep, and_mask,
                       N, out);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_gallery_split_bf16(const float *gallery, int64_t N, int E, void *hi, void *lo, float *resid_bound_out,
                                      void *stream)
{
    MMR_CHECK_ARG(N >= 0 && E >= 8 && E % 8 == 0, "mmr_gallery_split_bf16: bad shape N=%lld E=%d", (long long)N, E);
    if (N == 0) return MMR_OK;
    MMR_CHECK_ARG(gallery && hi && lo, "mmr_gallery_split_bf16: null pointer");
    MMR_CHECK_ARG((((uintptr_t)gallery | (uintptr_t)hi | (uintptr_t)lo) & 15) == 0, "mmr_gallery_split_bf16: pointers must be 16-byte aligned");
    const int64_t n8 = N * (E / 8);
    MMR_CHECK_ARG((n8 + 255) / 256 < 0x7fffffff, "mmr_gallery_split_bf16: gallery too large for one launch");
    hipLaunchKernelGGL(split_gallery_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gallery, n8,
                       (bf16_t *)hi, (bf16_t *)lo);
    MMR_CHECK_LAUNCH();
    if (resid_bound_out) {
        MMR_CHECK_HIP(hipMemsetAsync(resid_bound_out, 0, sizeof(float), (hipStream_t)stream));
        hipLaunchKernelGGL(split_resid_max_kernel, dim3(grid_1d(N, 4)), dim3(256), 0, (hipStream_t)stream,
                           gallery, (const bf16_t *)hi, N, E, (unsigned int *)resid_bound_out);
        MMR_CHECK_LAUNCH();
    }
    return MMR_OK;
}

extern "C" int mmr_cosine_topk_split(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                     const float *split_resid_bound_dev, int Q, int64_t N, int E, int k, float scale,
                                     float gallery_norm_bound, const float *gallery_norm_bound_dev, int32_t *idx, float *score,
                                     double *dot64, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    MMR_CHECK_ARG((gallery_hi && gallery_lo) || N == 0, "mmr_cosine_topk_split: null split arrays");
    MMR_CHECK_ARG((((uintptr_t)gallery_hi | (uintptr_t)gallery_lo) & 15) == 0, "mmr_cosine_topk_split: split arrays must be 16-byte aligned");
    return cosine_topk_impl(q, gallery, MMR_F32, Q, N, E, k, scale, gallery_norm_bound, gallery_norm_bound_dev, idx, score, dot64,
                            status, workspace, workspace_bytes, stream, (const bf16_t *)gallery_hi, (const bf16_t *)gallery_lo,
                            split_resid_bound_dev);
}

extern "C" int mmr_cosine_topk_split_masked(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                            const float *split_resid_bound_dev, int Q, int64_t N, int E, int k, float scale,
                                            float gallery_norm_bound, const float *gallery_norm_bound_dev, const uint32_t *row_mask,
                                            int32_t *idx, float *score, double *dot64, int32_t *status, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    MMR_CHECK_ARG((gallery_hi && gallery_lo) || N == 0, "mmr_cosine_topk_split: null split arrays");
    MMR_CHECK_ARG((((uintptr_t)gallery_hi | (uintptr_t)gallery_lo) & 15) == 0, "mmr_cosine_topk_split: split arrays must be 16-byte aligned");
    return cosine_topk_impl(q, gallery, MMR_F32, Q, N, E, k, scale, gallery_norm_bound, gallery_norm_bound_dev, idx, score, dot64,
                            status, workspace, workspace_bytes, stream, (const bf16_t *)gallery_hi, (const bf16_t *)gallery_lo,
                            split_resid_bound_dev, row_mask);
}

extern "C" int mmr_similarity(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, float scale,
                              float *out, void *stream)
{
    MMR_TRY(EntryCheck{"mmr_similarity"}.dtype(dtype));
    MMR_CHECK_ARG(Q >= 0 && N >= 0, "mmr_similarity: negative size");
    if (Q == 0 || N == 0) return MMR_OK;
    MMR_CHECK_ARG(q && gallery && out, "mmr_similarity: null pointer");
    MMR_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)gallery & 15) == 0, "mmr_similarity: q/gallery must be 16-byte aligned");
    MMR_CHECK_ARG((N + 3) / 4 < 0x7fffffff, "mmr_similarity: N too large");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 3) / 4));
    MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return dispatch_per(E, [&](auto per) -> int {
            hipLaunchKernelGGL((similarity_kernel<T, decltype(per)::value>), grid, dim3(256), 0, st, (const T *)q, (const T *)gallery, Q,
                               N, scale, out);
            return MMR_OK;
        });
    }));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_l2norm_rows(void *x, mmr_dtype dtype, int64_t rows, int E, void *stream)
{
    MMR_TRY(EntryCheck{"mmr_l2norm_rows"}.dtype(dtype));
    MMR_CHECK_ARG(rows >= 0 && E >= 1, "mmr_l2norm_rows: bad shape rows=%lld E=%d", (long long)rows, E);
    if (rows == 0) return MMR_OK;
    MMR_CHECK_ARG(x != nullptr, "mmr_l2norm_rows: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + 3) / 4));
    dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(l2norm_kernel<T>, grid, dim3(256), 0, st, (T *)x, rows, E);
        return 0;
    });
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_topk_merge(const int64_t *idx_parts, const double *dot_parts, int parts, int Q, int k, float scale,
                              int64_t *idx, float *score, double *dot64, void *stream)
{
    MMR_CHECK_ARG(parts >= 1 && Q >= 0 && k >= 1 && k <= K_MAX, "mmr_topk_merge: bad shape parts=%d Q=%d k=%d", parts, Q, k);
    MMR_CHECK_ARG(scale > 0.f, "mmr_topk_merge: scale must be > 0");
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(idx_parts && dot_parts && idx && score, "mmr_topk_merge: null pointer");
    MMR_CHECK_ARG(parts * k <= 1024, "mmr_topk_merge: parts*k=%d exceeds 1024", parts * k);
    hipLaunchKernelGGL(merge_kernel<false>, dim3(Q), dim3(64), 0, (hipStream_t)stream, idx_parts, dot_parts, parts, Q, k,
                       scale, idx, score, dot64);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_topk_pack(const int32_t *idx, const double *dot64, int Q, int k, int64_t row_offset, int64_t *packed,
                             void *stream)
{
    MMR_CHECK_ARG(Q >= 0 && k >= 1 && k <= K_MAX, "mmr_topk_pack: bad shape Q=%d k=%d", Q, k);
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(idx && dot64 && packed, "mmr_topk_pack: null pointer");
    const int n = Q * k;
    hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, dot64, row_offset, n, packed);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_topk_merge_packed(const int64_t *packed_parts, int parts, int Q, int k, float scale, int64_t *idx,
                                     float *score, double *dot64, void *stream)
{
    MMR_CHECK_ARG(parts >= 1 && Q >= 0 && k >= 1 && k <= K_MAX, "mmr_topk_merge_packed: bad shape parts=%d Q=%d k=%d", parts, Q, k);
    MMR_CHECK_ARG(scale > 0.f, "mmr_topk_merge_packed: scale must be > 0");
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(packed_parts && idx && score, "mmr_topk_merge_packed: null pointer");
    MMR_CHECK_ARG(parts * k <= 1024, "mmr_topk_merge_packed: parts*k=%d exceeds 1024", parts * k);
    hipLaunchKernelGGL(merge_kernel<true>, dim3(Q), dim3(64), 0, (hipStream_t)stream, packed_parts, (const double *)nullptr,
                       parts, Q, k, scale, idx, score, dot64);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_tip_adapter_logits(const void *features, const void *clip_weights_t, const void *cache_keys_t,
                                      const float *cache_values, mmr_dtype dtype, int64_t N, int E, int C, int S,
                                      float alpha, float beta, float *tip_logits, float *clip_logits, void *stream)
{
    MMR_TRY(EntryCheck{"mmr_tip_adapter_logits"}.dtype(dtype));
    MMR_CHECK_ARG(N >= 0 && C >= 1 && C <= 64 && S >= 0, "mmr_tip_adapter_logits: bad shape N=%lld C=%d S=%d (C <= 64)", (long long)N, C, S);
    if (N == 0) return MMR_OK;
    MMR_CHECK_ARG(features && clip_weights_t && tip_logits && (S == 0 || (cache_keys_t && cache_values)), "mmr_tip_adapter_logits: null pointer");
    MMR_CHECK_ARG((((uintptr_t)features | (uintptr_t)clip_weights_t | (uintptr_t)cache_keys_t) & 15) == 0, "mmr_tip_adapter_logits: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 3) / 4));
    MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return dispatch_per(E, [&](auto per) -> int {
            hipLaunchKernelGGL((tip_logits_kernel<T, decltype(per)::value>), grid, dim3(256), 0, st, (const T *)features,
                               (const T *)clip_weights_t, (const T *)cache_keys_t, cache_values, N, C, S, alpha, beta, tip_logits,
                               clip_logits);
            return MMR_OK;
        });
    }));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
