// The top-k scans over 16-bit operands: scan_body / scan16_body, the kernels scan_kernel / scan16_kernel around them and
// their launcher.  T (ET) is the element type of the queries and the gallery, bf16_t or f16_t; it picks the MFMA
// instruction (scan_pipeline.h: mfma_32x32x16 / mfma_16x16x32) and nothing else: the staging, the ring, the waits and the
// bucket maxima are the same code.  search.hip instantiates the bf16 kernels, search_f16.hip the fp16 ones; the per-query
// kernels around the same bodies are deep_qmask.hip's.  The bodies are force-inlined.
#pragma once
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "scan_host.h"
#include "topk_scan.h"

#include <math.h>

namespace mmr {

constexpr int TILE_ROWS = 32;
#ifndef MMR_SCAN_NBUF
#define MMR_SCAN_NBUF 3
#endif
constexpr int SCAN_NBUF = MMR_SCAN_NBUF;
#ifndef MMR_SCAN_CHAINS_FOR
#define MMR_SCAN_CHAINS_FOR(waves) chains_32x32(waves)   // independent MFMA accumulation chains per wave
#endif
#ifndef MMR_SCAN_PF
#define MMR_SCAN_PF 4                                     // k-steps the A fragment reads run ahead of the MFMAs
#endif
static_assert(SCAN_NBUF == 3 || SCAN_NBUF == 4, "wait counts below assume a prefetch distance of 2 or 3 tiles");

// ---------------------------------------------------------------------------------------------
// QMASK: a row mask per query (mmr_cosine_topk_deep_qmasked; the kernels are deep_qmask.hip's).  The tile's word is no
// longer wave-uniform, so the readlane of row_mask_tile32 does not serve: the task's words are staged ONCE, before the
// ring, into LDS behind the ring's slots as words[tile - t0][query], QMASK_PAD words between tile rows, with the shared
// mask AND-ed in and the bits at or past N cleared.  Each lane then reads its query's word of tile t with one
// ds_read_b32 issued IN FRONT of the tile's k-loop: LDS reads return in order, so every counted lgkmcnt wait of the
// k-loop covers it as well, and the k-loop's last wait (lgkmcnt(0)) has it landed; the epilogue names it in one more
// lgkmcnt(0), which costs nothing there.  Nothing is loaded from memory inside the ring.
// ---------------------------------------------------------------------------------------------
// QMaskArgs: scan_pipeline.h
// words between the LDS rows of two tiles: qpad + 1, so that the staging's writes (lanes = tiles, one query) fall into
// different banks; the epilogue's reads (lanes = queries, one tile) are consecutive anyway
constexpr int QMASK_PAD = 1;
__host__ __device__ constexpr int qmask_lds_bytes(int tpt, int qpad) { return tpt * (qpad + QMASK_PAD) * 4; }

// Stage the words of the tiles [t0, t1) (at most 64: one per lane) for the queries [0, qpad).  A wave reads 64
// consecutive words of one query's row (coalesced), four queries in flight; queries at or past Q get 0.
template <int WAVES>
__device__ __forceinline__ void qmask_stage(uint32_t *__restrict__ words, const QMaskArgs &qm, int Q, int qpad, int t0, int t1,
                                            int64_t N, int wave, int lane)
{
    const int t = t0 + lane;
    const bool in = t < t1;
    uint32_t sh = 0u;
    if (in) {
        sh = qm.shared ? qm.shared[t] : 0xffffffffu;
        const int64_t left = N - (int64_t)t * TILE_ROWS;
        if (left < 32) sh &= (1u << (int)left) - 1u;
    }
    const uint32_t *src = qm.row_masks + (in ? t : t0);
    uint32_t *dst = words + lane * (qpad + QMASK_PAD);
    for (int q0 = wave * 4; q0 < qpad; q0 += WAVES * 4) {       // qpad is a multiple of 32
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = q0 + j < Q ? src[(size_t)(q0 + j) * qm.stride] : 0u;
        if (in) {
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[q0 + j] = w[j] & sh;
        }
    }
}
__device__ __forceinline__ void ds_read_b32(uint32_t &dst, const void *lds)
{
    asm volatile("ds_read_b32 %0, %1" : "=v"(dst) : "v"((uint32_t)(uintptr_t)lds));
}

// ---------------------------------------------------------------------------------------------
// scan (E <= 512): the 32x32x16 form of scan_pipeline.h, 8 waves x 32 queries
// ---------------------------------------------------------------------------------------------
template <int E>
struct ScanCfg : Tile32<E> {
    static_assert(E <= 512, "E = 768 runs scan16_kernel");
    static constexpr int QMAX = Tile32<E>::WAVES * 32;      // queries per scan pass
    static constexpr int KSTEPS = E / 16;
    static constexpr int LDS = SCAN_NBUF * Tile32<E>::TILE_BYTES;
};

// MASKED: row_mask (scan_pipeline.h) drops rows from the bucket maxima; a dead tile's maximum is -inf.
// QMASK (with MASKED = false): the per-query masks `qm` above; row_mask is not read.
template <class T, int E, bool MASKED, bool QMASK = false>
__device__ __forceinline__ void scan_body(
    const T *__restrict__ q, const T *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask,
    const QMaskArgs qm = {})
{
    static_assert(!(MASKED && QMASK), "the shared mask of a per-query scan travels in QMaskArgs");
    using C = ScanCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int task = blockIdx.x;
    const int t0 = task * tpt;
    const int t1 = min(ntiles, t0 + tpt);
    const bool compute = wave < qwaves;

    // B operand: this wave's 32 queries, resident for the whole task.  Lane (c,h) holds, for
    // k-step s, the 8 elements [16s + 8h, 16s + 8h + 8) of query wave*32 + c.
    const MaskWord mw = MASKED ? mask_issue(row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    {
        const int qrow = wave * 32 + c;
        const bool live = compute && qrow < Q;
        load_query_b16<C::KSTEPS, 16>(q + (size_t)(live ? qrow : 0) * E + h * 8, live, bq);
    }
    const uint32_t mwords = mask_take(mw);
    if constexpr (QMASK) {
        qmask_stage<C::WAVES>((uint32_t *)(smem + C::LDS), qm, Q, qpad, t0, t1, N, wave, lane);
        __syncthreads();
    }
    BucketMax bm{bmax, qpad, wave * 32 + c, compute, h == 0};
    tile_ring<SCAN_NBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(gal, gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { bm.flush(); },
        [&](int t, int cur) {
            if (!compute) return;
            uint32_t qw = 0u;
            if constexpr (QMASK) ds_read_b32(qw, smem + C::LDS + ((t - t0) * (qpad + QMASK_PAD) + wave * 32 + c) * 4);
            const f32x16 acc = tile_dot_32x32<E, MMR_SCAN_CHAINS_FOR(C::WAVES), MMR_SCAN_PF, T>(
                smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);
            // acc[i] = dot(query c, tile row (i&3) + 8*(i>>2) + 4*h)
            float m = -INFINITY;
            if constexpr (QMASK) {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qw));
                const uint32_t wh = qw >> (4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i) m = fmaxf(m, (wh >> ((i & 3) + 8 * (i >> 2))) & 1u ? acc[i] : -INFINITY);
            } else if constexpr (MASKED) {
                const uint32_t w = row_mask_tile32(mwords, t, t0, N);
                if (w == 0xffffffffu) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) m = fmaxf(m, acc[i]);
                } else {
                    const uint32_t wh = w >> (4 * h);
#pragma unroll
                    for (int i = 0; i < 16; ++i) m = fmaxf(m, (wh >> ((i & 3) + 8 * (i >> 2))) & 1u ? acc[i] : -INFINITY);
                }
            } else if ((int64_t)(t + 1) * TILE_ROWS <= N) {
#pragma unroll
                for (int i = 0; i < 16; ++i) m = fmaxf(m, acc[i]);
            } else {
                const int64_t base = (int64_t)t * TILE_ROWS + 4 * h;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t r = base + (i & 3) + 8 * (i >> 2);
                    m = fmaxf(m, r < N ? acc[i] : -INFINITY);
                }
            }
            bm.add(t, fmaxf(m, __shfl_xor(m, 32, 64)));
        });
    bm.finish(tmax, task);
}

// ---------------------------------------------------------------------------------------------
// scan for wide rows (E = 768, the ViT-L/14 embedding; BASELINE configs[4]).  32 resident queries of 768 dims are 192
// VGPRs, which forced the 32x32 form down to one wave per SIMD with the queries parked in AccVGPRs and copied back in
// front of every MFMA (0.33 of the HBM roof).  Here each of 8 waves keeps 16 queries (96 VGPRs) and multiplies with
// v_mfma_f32_16x16x32_bf16: the same 128 queries per pass, but two waves per SIMD (one reads LDS while the other issues
// MFMAs), no register shuffling, and the 16x16 shape's higher sustained clock.  A 32-row tile is two 16-row blocks with
// one accumulation chain each.  Same LDS image, staging ring, counted waits and bmax/tmax outputs as scan_kernel, so the
// finalize kernels do not care which scan ran.
//   B operand: lane (c = lane & 15, g = lane >> 4) holds elements [32s + 8g, +8) of query wave*16 + c for k-step s;
//   A operand: the same 8 elements of tile row 16*rb + c;  D: acc[i] = dot(query c, tile row 16*rb + 4g + i).
// Bank check for the A reads (ds_read_b128, 16-lane groups {0-3,12-15,20-27} ...): a group's lanes read rows
// {0-3,12-15} at chunk 4s and rows {4-11} at chunk 4s+1; slot = (chunk ^ row) & 15 gives 16 distinct slots.
// ---------------------------------------------------------------------------------------------
template <int E>
struct Scan16Cfg : TileGeom<E, 2, TILE_ROWS, 8> {
    static constexpr int QMAX = 8 * 16;               // 128 queries per scan pass
    static constexpr int KSTEPS = E / 32;
    static constexpr int LDS = SCAN_NBUF * Scan16Cfg::TILE_BYTES;
};

template <class T, int E, bool MASKED, bool QMASK = false>
__device__ __forceinline__ void scan16_body(
    const T *__restrict__ q, const T *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask,
    const QMaskArgs qm = {})
{
    static_assert(!(MASKED && QMASK), "the shared mask of a per-query scan travels in QMaskArgs");
    using C = Scan16Cfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int task = blockIdx.x;
    const int t0 = task * tpt;
    const int t1 = min(ntiles, t0 + tpt);
    const bool compute = wave < qwaves;

    const MaskWord mw = MASKED ? mask_issue(row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    {
        const int qrow = wave * 16 + c;
        const bool live = compute && qrow < Q;
        load_query_b16<C::KSTEPS, 32>(q + (size_t)(live ? qrow : 0) * E + g * 8, live, bq);
    }
    const uint32_t mwords = mask_take(mw);
    if constexpr (QMASK) {
        qmask_stage<8>((uint32_t *)(smem + C::LDS), qm, Q, qpad, t0, t1, N, wave, lane);
        __syncthreads();
    }
    BucketMax bm{bmax, qpad, wave * 16 + c, compute, g == 0};
    tile_ring<SCAN_NBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(gal, gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { bm.flush(); },
        [&](int t, int cur) {
            if (!compute) return;
            const char *tb = smem + cur * C::TILE_BYTES;
            // step u = 2*s + rb: k-step s of row block rb; the two row blocks alternate, so consecutive MFMAs belong to
            // different accumulation chains.  Fragment reads run PF steps ahead (scan_pipeline.h: wait_lgkmcnt).
            constexpr int NU = 2 * C::KSTEPS;
            constexpr int PF = 6;
            f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
            bf16x8 a[PF];
            uint32_t qw = 0u;
            if constexpr (QMASK) ds_read_b32(qw, smem + C::LDS + ((t - t0) * (qpad + QMASK_PAD) + wave * 16 + c) * 4);
            auto issue = [&](int u, bf16x8 &dst) {
                const int row = (u & 1) * 16 + c;
                ds_read_b128(dst, tb + row * C::ROWB + swizzle(4 * (u >> 1) + g, row) * 16);
            };
#pragma unroll
            for (int u = 0; u < PF; ++u) issue(u, a[u]);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                wait_lgkmcnt((NU - 1 - u) < (PF - 1) ? (NU - 1 - u) : (PF - 1), a[u % PF]);
                if (u & 1) acc1 = mfma_16x16x32<T>(a[u % PF], bq[u >> 1], acc1);
                else acc0 = mfma_16x16x32<T>(a[u % PF], bq[u >> 1], acc0);
                if (u + PF < NU) {
                    // the MFMA above must have read a[u % PF] before the next load overwrites it
                    if (u & 1) asm volatile("" : "+v"(acc1)); else asm volatile("" : "+v"(acc0));
                    issue(u + PF, a[u % PF]);
                }
            }
            // acc0[i] = dot(query c, tile row 4g + i); acc1[i]: tile row 16 + 4g + i
            float m = -INFINITY;
            uint32_t w = 0xffffffffu;
            if constexpr (MASKED) w = row_mask_tile32(mwords, t, t0, N);
            if constexpr (QMASK) {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qw));
                w = qw;
            }
            if (QMASK || (MASKED && w != 0xffffffffu)) {
                const uint32_t wg = w >> (4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    m = fmaxf(m, (wg >> i) & 1u ? acc0[i] : -INFINITY);
                    m = fmaxf(m, (wg >> (16 + i)) & 1u ? acc1[i] : -INFINITY);
                }
            } else if (MASKED || (int64_t)(t + 1) * TILE_ROWS <= N) {
                m = fmaxf(fmaxf(fmaxf(acc0[0], acc0[1]), fmaxf(acc0[2], acc0[3])),
                          fmaxf(fmaxf(acc1[0], acc1[1]), fmaxf(acc1[2], acc1[3])));
            } else {
                const int64_t base = (int64_t)t * TILE_ROWS + 4 * g;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    m = fmaxf(m, base + i < N ? acc0[i] : -INFINITY);
                    m = fmaxf(m, base + 16 + i < N ? acc1[i] : -INFINITY);
                }
            }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            bm.add(t, fmaxf(m, __shfl_xor(m, 32, 64)));
        });
    bm.finish(tmax, task);
}

// ---------------------------------------------------------------------------------------------
// The kernels: scan_kernel (E <= 512) is the 32x32x16 form of scan_pipeline.h, 8 waves x 32 queries; scan16_kernel
// (E = 768) the 16x16x32 form, 8 waves x 16 queries.
// MASKED: row_mask (scan_pipeline.h) drops rows from the bucket maxima; a dead tile's maximum is -inf.
// ---------------------------------------------------------------------------------------------
template <typename ET, int E, bool MASKED>
__global__ __launch_bounds__(ScanCfg<E>::THREADS, ScanCfg<E>::WAVES / 4) void scan_kernel(
    const ET *__restrict__ q, const ET *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask)
{
    scan_body<ET, E, MASKED>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, row_mask);
}

template <typename ET, int E, bool MASKED>
__global__ __launch_bounds__(Scan16Cfg<E>::THREADS, 2) void scan16_kernel(
    const ET *__restrict__ q, const ET *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask)
{
    scan16_body<ET, E, MASKED>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, row_mask);
}

// The scan of one query chunk over 16-bit operands: the 32x32 form up to E = 512, scan16_kernel at E = 768.  row_mask NULL:
// the unmasked kernels.
template <typename ET>
int launch_topk_scan_16(int E, const ET *q, const ET *gal, int Qc, int64_t N, const TopkScanGeom &g, int qpad, float *bmax,
                        float *tmax, const uint32_t *row_mask, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        return dispatch_masked(row_mask, [&](auto m) -> int {
            constexpr int EE = decltype(e)::value;
            constexpr bool MASKED = decltype(m)::value;
            if constexpr (EE == 768)
                return launch_scan_kernel<&scan16_kernel<ET, EE, MASKED>>(g.ntasks, Scan16Cfg<EE>::THREADS, Scan16Cfg<EE>::LDS, st, q,
                                                                          gal, Qc, N, g.ntiles, g.tpt, qpad / 16, qpad, bmax, tmax,
                                                                          row_mask);
            else
                return launch_scan_kernel<&scan_kernel<ET, EE, MASKED>>(g.ntasks, ScanCfg<EE>::THREADS, ScanCfg<EE>::LDS, st, q, gal,
                                                                        Qc, N, g.ntiles, g.tpt, qpad / 32, qpad, bmax, tmax, row_mask);
        });
    });
}
// the fp16 kernels: search_f16.hip
extern template int launch_topk_scan_16<f16_t>(int, const f16_t *, const f16_t *, int, int64_t, const TopkScanGeom &, int, float *,
                                               float *, const uint32_t *, hipStream_t);

}  // namespace mmr
