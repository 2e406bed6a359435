// sweep_scan_kernel, the scan of the labelled threshold sweep (sweep.hip), with its geometry, arguments and launcher.  One
// kernel template over the element type ET, bf16_t or f16_t (range_scan_body.h says why a template), with or without a
// row mask per query; sweep.hip instantiates the bf16 kernels, sweep_f16.hip the fp16 ones, sweep_qmask.hip the
// per-query ones of both types.
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
    // 16-bit elements: bf16, or fp16 for sweep_scan_kernel<f16_t> (the caller casts)
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

// the kernel's optional last argument, or none
__device__ __forceinline__ QMaskArgs sweep_qmask_args() { return {}; }
__device__ __forceinline__ QMaskArgs sweep_qmask_args(const QMaskArgs &qm) { return qm; }

// ET: the element type behind a.q / a.gal -- it picks the MFMA instruction (scan_pipeline.h) and how the resident query's
// norm is read.  QM: empty, or QMaskArgs -- the kernel then takes a second argument, a row mask per query of the pass
// (QMASK), a.row_mask being NULL, MASKED false and the mask the queries share travelling in QMaskArgs.
template <typename ET, int E, bool MASKED, typename... QM>
__global__ __launch_bounds__(SweepCfg<E>::THREADS, SweepCfg<E>::WAVES / 4) void sweep_scan_kernel(SweepScanArgs a, QM... qmv)
{
    constexpr bool QMASK = sizeof...(QM) != 0;
    static_assert(!(MASKED && QMASK), "the shared mask of a per-query scan travels in QMaskArgs");
    const QMaskArgs qm = sweep_qmask_args(qmv...);
    using C = SweepCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;
    const int T = a.T;

    const int t0 = blockIdx.x * a.tpt;
    const int t1 = min(a.ntiles, t0 + a.tpt);

    // B operand: this wave's 32 queries (scan_kernel's layout)
    const int64_t gq = (int64_t)a.q0 + wave * 32 + c;
    const bool qlive = wave * 32 + c < a.Qc;
    const bool compute = wave * 32 < a.Qc;             // wave-uniform: this wave holds a live query
    // mask words of the tiles [t0, t1): issued in front of the query loads, taken behind them (scan_pipeline.h)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    double qn2 = 0.0;                  // fp64: a small query's squares underflow in fp32
    {
        const bf16_t *qp = a.q + (size_t)(qlive ? wave * 32 + c : 0) * E + h * 8;
        load_query_b16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = b16_to_f32<ET>((uint16_t)bq[s][j]); qn2 += x * x; }
    }
    qn2 += __shfl_xor(qn2, 32, 64);
    const uint32_t mwords = mask_take(mw);
    const int32_t tgt = a.targets[qlive ? gq : a.q0];

    const ScanMargin mg = scan_margin(qn2, a.host_bound, a.dev_bound, a.split, a.resid_dev, a.qres, qlive ? gq : a.q0);

    // LDS behind the ring: the labels of this task's rows, the fp32 grid, the resident queries' margin / target / flags
    // (bit 0 live, bit 1 wild), the (query, bin) counts, every wave's candidate staging
    const int nq = a.ncw * 32;
    int32_t *lab = (int32_t *)(smem + C::RING);
    float *down = (float *)(smem + C::RING + SWEEP_LABEL_BYTES);
    float *up = down + (T + 2);
    double *qeps = (double *)(smem + C::RING + SWEEP_LABEL_BYTES + sweep_grid_bytes(T));
    int32_t *qtgt = (int32_t *)(qeps + nq);
    uint32_t *qflag = (uint32_t *)(qtgt + nq);
    uint32_t *hist = qflag + nq;
    const int hwords = a.hrows * (T + 1);
    {
        const int nrows = (t1 - t0) * RTILE;
        for (int i = threadIdx.x; i < nrows; i += C::THREADS) {
            const int64_t r = (int64_t)t0 * RTILE + i;
            lab[i] = r < N ? a.labels[r] : 0;
        }
        for (int i = threadIdx.x; i < 2 * (T + 2); i += C::THREADS) down[i] = a.grid32[i];
        for (int i = threadIdx.x; i < hwords; i += C::THREADS) hist[i] = 0u;
        if (wave < a.ncw && h == 0) {            // every entry the binning can read, dead queries included (flags 0)
            qeps[wave * 32 + c] = mg.eps;
            qtgt[wave * 32 + c] = tgt;
            qflag[wave * 32 + c] = (qlive ? 1u : 0u) | (mg.wild ? 2u : 0u);
        }
    }
    // this wave's candidate staging (wave-private: LDS operations of one wave execute in order, so no barrier)
    const int scap = a.stage;
    uint64_t *stg = (uint64_t *)(hist + hwords + (hwords & 1)) + (size_t)wave * scap;
    // QMASK: behind the staging, the mask words of this task's tiles for the pass's queries, [tile][hrows + 1], the shared
    // mask AND-ed in and the bits at or past N cleared; threads run along a query's row (coalesced)
    const uint32_t *qmw = (const uint32_t *)((uint64_t *)(hist + hwords + (hwords & 1)) + (size_t)C::WAVES * scap);
    const int qmstride = a.hrows + 1;
    if constexpr (QMASK) {
        uint32_t *wr = (uint32_t *)((uint64_t *)(hist + hwords + (hwords & 1)) + (size_t)C::WAVES * scap);
        const int nt = t1 - t0;
        for (int i = threadIdx.x; i < nt * a.Qc; i += C::THREADS) {
            const int qi = i / nt, tl = i - qi * nt;
            uint32_t w = qm.row_masks[(size_t)qi * qm.stride + t0 + tl];
            if (qm.shared) w &= qm.shared[t0 + tl];
            const int64_t left = N - (int64_t)(t0 + tl) * RTILE;
            if (left < 32) w &= (1u << (int)left) - 1u;
            wr[tl * qmstride + qi] = w;
        }
    }
    int nst = 0;
    const float gt0 = a.gt0, ginv = a.ginv, Tf = (float)T;
    unsigned long long *counter = a.counter;
    uint64_t *cand = a.cand;
    const int64_t cand_cap = a.cand_cap;
    const bf16_t *gal = a.gal;
    const int ncw = a.ncw, q0 = a.q0;
    const int nel = ncw * (1024 / C::THREADS);       // accumulator elements per thread and tile
    __syncthreads();

    tile_ring<C::NBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(gal, gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [] {},
        [&](int t, int cur) {
            char *slot = smem + cur * C::TILE_BYTES;
            f32x16 acc;
            if (compute) acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(slot + c * C::ROWB, c, h, bq);
            // One wave multiplies for 32 queries; ALL waves bin.  The products change hands through the tile's own slot,
            // which is free once every multiplying wave has read it and until the ring stages into it again, behind the
            // next tile's barrier: [wave][row][query] fp32, 4 KiB per multiplying wave (SweepCfg::QCAP keeps that inside
            // the slot).  Raw barriers and LDS-only waits: a vmcnt wait here would drain the ring's prefetch.
            if (ncw > 1) __builtin_amdgcn_s_barrier();
            if (compute) {
                float *ab = (float *)slot + wave * 1024 + 4 * h * 32 + c;
#pragma unroll
                for (int i = 0; i < 16; ++i) ab[((i & 3) + 8 * (i >> 2)) * 32] = acc[i];      // row (i&3) + 8*(i>>2) + 4h
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");

            // element e = thread + k * THREADS of the tile's products: wave e >> 10, row (e >> 5) & 31, query e & 31 = c
            const float *ab = (const float *)slot + threadIdx.x;
            const uint32_t wrow = MASKED ? row_mask_tile32(mwords, t, t0, N) : 0u;
            const int32_t *lt = lab + (t - t0) * RTILE;
            const int64_t base = (int64_t)t * RTILE;
            uint32_t pred = 0;
#pragma unroll 2
            for (int k = 0; k < nel; ++k) {
                const int e = threadIdx.x + k * C::THREADS;
                const int qi = (e >> 10) * 32 + c, r = (e >> 5) & 31;
                const float av = ab[k * C::THREADS];
                const uint32_t fl = qflag[qi];
                const double eps = qeps[qi];
                bool live;
                if constexpr (QMASK) live = (fl & 1u) && ((qmw[(t - t0) * qmstride + ((fl & 1u) ? qi : 0)] >> r) & 1u);
                else live = (fl & 1u) && (MASKED ? ((wrow >> r) & 1u) : base + r < N);
                // [lo, hi] holds the exact dot (bounds rounded outward)
                const float hi = f32_up((double)av + eps), lo = f32_down((double)av - eps);
                // b = #{j : down[j] <= hi} >= the exact dot's bin; guessed for an even grid, confirmed by two reads
                int b = (int)fminf(fmaxf((hi - gt0) * ginv + 1.f, 0.f), Tf);
                if (!(down[b] <= hi && hi < down[b + 1])) {
                    int l = 0, u = T;
                    for (int it = 0; it < 11; ++it) {
                        const int mid = (l + u + 1) >> 1;
                        const bool ge = l < u && down[mid] <= hi;
                        u = (l < u && !ge) ? mid - 1 : u;
                        l = ge ? mid : l;
                    }
                    b = l;
                }
                // #{j : up[j] <= lo} <= the exact dot's bin, and it reaches b iff up[b] <= lo: then the bin is b
                const bool decided = !(fl & 2u) && fabsf(av) < INFINITY && up[b] <= lo;
                if (live) {
                    if (decided) atomicAdd(hist + qi * (T + 1) + b, lt[r] == qtgt[qi] ? 0x10000u : 1u);
                    else pred |= 1u << k;
                }
            }
            const int n = __popc(pred);
            const WavePrefix wp = wave_prefix(n, lane);
            if (nst + wp.total > scap) {
                flush_staged(stg, nst, lane, counter, cand, cand_cap);
                nst = 0;
            }
            if (wp.total > 0) {
                // more than the staging holds (a wild query: every pair): straight to the list
                const bool direct = wp.total > scap;
                unsigned long long wbase = 0;
                if (direct) {
                    if (lane == 0) wbase = atomicAdd(counter, (unsigned long long)wp.total);
                    wbase = __shfl(wbase, 0, 64);
                }
                unsigned long long pos = wbase + (unsigned long long)wp.before;
                uint64_t *dst = stg + nst + wp.before;
                for (int k = 0; k < nel; ++k) {
                    if (pred & (1u << k)) {
                        const int e = threadIdx.x + k * C::THREADS;
                        const uint64_t key = ((uint64_t)(q0 + (e >> 10) * 32 + c) << 32) | (uint64_t)(base + ((e >> 5) & 31));
                        if (!direct) *dst++ = key;
                        else if (pos < (unsigned long long)cand_cap) cand[pos] = key;
                        ++pos;
                    }
                }
                if (!direct) nst += wp.total;
            }
        });
    flush_staged(stg, nst, lane, counter, cand, cand_cap);

    // flush: low half = rows of another label, high half = rows of the query's label (a task has at most 2048 rows)
    __syncthreads();
    for (int i = threadIdx.x; i < hwords; i += C::THREADS) {
        const uint32_t w = hist[i];
        if (w) {
            const int qr = i / (T + 1), b = i - qr * (T + 1);
            unsigned long long *g = a.hist + ((size_t)(a.q0 + qr) * 2) * (T + 1) + b;
            if (w & 0xffffu) atomicAdd(g, (unsigned long long)(w & 0xffffu));
            if (w >> 16) atomicAdd(g + (T + 1), (unsigned long long)(w >> 16));
        }
    }
}

// One pass with `lds` bytes of LDS (sweep.hip plans them).  a.row_mask NULL: the unmasked kernels.
template <typename ET>
int launch_sweep_scan(int E, const SweepScanArgs &a, unsigned grid, int lds, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        if (a.row_mask) return launch_scan_kernel_lds<&sweep_scan_kernel<ET, decltype(e)::value, true>>(grid, C::THREADS, lds, SWEEP_LDS_MAX, st, a);
        return launch_scan_kernel_lds<&sweep_scan_kernel<ET, decltype(e)::value, false>>(grid, C::THREADS, lds, SWEEP_LDS_MAX, st, a);
    });
}
// the fp16 kernels: sweep_f16.hip
extern template int launch_sweep_scan<f16_t>(int, const SweepScanArgs &, unsigned, int, hipStream_t);
// sweep_qmask.hip: the pass with a mask row per query (qm.row_masks: the pass's first query's row), bf16 or fp16 elements
int launch_sweep_scan_qmasked(int E, bool f16, const SweepScanArgs &a, const QMaskArgs &qm, unsigned grid, int lds, hipStream_t st);

}  // namespace mmr
