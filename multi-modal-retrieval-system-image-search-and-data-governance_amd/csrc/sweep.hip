// Labelled threshold sweep for gfx950 (MI355X): exact TP / FP counts at every point of a threshold grid, one pass.
//
// Replaces the tail every retrieval driver of the reference shares -- score the gallery against a few class vectors,
// split the scores by label, count `pos >= t` and `neg >= t` over a grid --
//     eval_threshold / find_thresholds      reference code/search_image.py:39-103, code/main_custom.py:27-92
//     evaluate_thresholds                   reference CLIP/lab3.py:39-65, CLIP/union_dataset.py:46-61
// without the [Q,N] score matrix and without one range search per grid point.
//
// Structure ("Threshold sweep"):
//   sweep_scan_kernel<E, MASKED>   range_scan_kernel's pipeline (scan_pipeline.h: queries resident as MFMA B fragments,
//                                  LDS ring filled by global_load_lds, counted waits) with a binning epilogue.  With
//                                  a = the approximate dot and eps = margin(query) (range_common.h), a pair is
//                                    DECIDED    when no threshold lies in [a - eps, a + eps]: the exact dot has a's bin,
//                                               bin = #{i : thresholds[i] <= a}; one LDS atomic on the workgroup's
//                                               histogram word (query, bin): negatives in the low half, positives in
//                                               the high half;
//                                    AMBIGUOUS  otherwise (or a is not finite, or the query is wild): a candidate,
//                                               (query << 32) | row, as in range_scan_kernel.  A grid makes candidates
//                                               common (the share of pairs within eps of a grid point), and a
//                                               returning global atomic inside the ring drains its prefetch, so each
//                                               wave stages its candidates in LDS and appends them in batches: one
//                                               64-bit atomicAdd per batch, the counter runs past the capacity.
//                                  When the task ends the non-zero words go to the global int64 histogram.
//   sweep_recheck_kernel           exact fp64 dot (quad_dot on the ORIGINAL rows) of every stored candidate, NaN dropped,
//                                  bin by binary search over the fp64 grid, one global atomic.
//   sweep_finish_kernel            hist[Q,2,T+1] -> ge (suffix sums), total (row sums), counts.
// Integer atomics only: the result does not depend on arrival order.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "range_common.h"

#include <math.h>

#include <hip/hip_runtime.h>

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

// LDS left for the counts and the candidate staging
static int sweep_lds_room(int E, int T)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        return SWEEP_LDS_MAX - C::RING - SWEEP_LABEL_BYTES - sweep_grid_bytes(T);
    });
}
static int sweep_hist_bytes(int rows, int T) { return (rows * (T + 1) * 4 + 7) / 8 * 8; }      // the staging behind it is 8-byte aligned
static int sweep_waves(int E) { return E <= 512 ? 8 : 4; }
// per-query margin / target / flags (16 B) of the multiplying waves, the counts, every wave's staging
static int sweep_lds_need(int E, int rows, int T, int stage)
{
    return (rows + 31) / 32 * 32 * 16 + sweep_hist_bytes(rows, T) + sweep_waves(E) * stage * 8;
}

// queries per gallery pass: what fits in LDS beside the ring, the labels and the grid (their counts plus the least
// staging for each wave that multiplies), at most the kernel's QMAX
static int sweep_queries_per_pass(int E, int T)
{
    const int room = sweep_lds_room(E, T);
    int rows = scan_dispatch_E(E, [&](auto e) { return (int)SweepCfg<decltype(e)::value>::QCAP; });
    while (rows > 1 && sweep_lds_need(E, rows, T, SWEEP_STAGE_MIN) > room) --rows;
    return rows;
}
// staging entries per wave when a pass holds `rows` queries: the LDS that is left, at most SWEEP_STAGE_MAX
static int sweep_stage_entries(int E, int T, int rows)
{
    const int left = (sweep_lds_room(E, T) - sweep_lds_need(E, rows, T, 0)) / sweep_waves(E) / 8;
    return left < SWEEP_STAGE_MAX ? left : SWEEP_STAGE_MAX;
}

struct SweepScanArgs {
    const bf16_t *q;                 // bf16 queries of this pass [Qc,E]
    const bf16_t *gal;               // bf16 gallery, or the hi half of an fp32 gallery
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

// (float)x rounded toward -inf / +inf
__device__ __forceinline__ float f32_down(double x)
{
    float f = (float)x;
    if ((double)f > x) {
        const uint32_t b = __float_as_uint(f);
        f = f > 0.f ? __uint_as_float(b - 1) : (f == 0.f ? __uint_as_float(0x80000001u) : __uint_as_float(b + 1));
    }
    return f;
}
__device__ __forceinline__ float f32_up(double x)
{
    float f = (float)x;
    if ((double)f < x) {
        const uint32_t b = __float_as_uint(f);
        f = f < 0.f ? __uint_as_float(b - 1) : (f == 0.f ? __uint_as_float(0x00000001u) : __uint_as_float(b + 1));
    }
    return f;
}

// The fp32 images of the grid the scan compares against, with sentinels: down[0] = up[0] = -inf,
// down[k] = thresholds[k-1] rounded down, up[k] = thresholds[k-1] rounded up, down[T+1] = up[T+1] = +inf.
// The grid arrives by value, SWEEP_CHUNK points per launch: the caller's host array is read before the call returns.
constexpr int SWEEP_CHUNK = 256;
struct SweepGridChunk {
    double t[SWEEP_CHUNK];
};
__global__ __launch_bounds__(SWEEP_CHUNK) void sweep_grid_kernel(SweepGridChunk ch, int off, int n, int T, double *__restrict__ thr64,
                                                                float *__restrict__ grid32)
{
    const int i = threadIdx.x;
    float *down = grid32, *up = grid32 + (T + 2);
    if (i < n) {
        const double t = ch.t[i];
        thr64[off + i] = t;
        down[off + i + 1] = f32_down(t);
        up[off + i + 1] = f32_up(t);
    }
    if (off == 0 && i == 0) {
        down[0] = -INFINITY; up[0] = -INFINITY;
        down[T + 1] = INFINITY; up[T + 1] = INFINITY;
    }
}

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

template <int E, bool MASKED>
__global__ __launch_bounds__(SweepCfg<E>::THREADS, SweepCfg<E>::WAVES / 4) void sweep_scan_kernel(SweepScanArgs a)
{
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
        load_query_bf16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = bf16_to_f32((bf16_t)bq[s][j]); qn2 += x * x; }
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
            if (compute) acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF>(slot + c * C::ROWB, c, h, bq);
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
                const bool live = (fl & 1u) && (MASKED ? ((wrow >> r) & 1u) : base + r < N);
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

// Exact recheck: one candidate per 16-lane group, quad_dot on the original rows (fp32 rows for an fp32 gallery).
// The fp64 grid sits in LDS (at most 8 KiB): the bin search is ten dependent reads per candidate.
template <typename T, int PER>
__global__ __launch_bounds__(256) void sweep_recheck_kernel(const T *__restrict__ q, const T *__restrict__ gal,
                                                            const int32_t *__restrict__ labels, const int32_t *__restrict__ targets,
                                                            const double *__restrict__ thr64, int nthr,
                                                            const unsigned long long *__restrict__ counter,
                                                            const uint64_t *__restrict__ cand, int64_t cand_cap,
                                                            unsigned long long *__restrict__ hist)
{
    constexpr int E = PER * 64;
    extern __shared__ double sthr[];
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, grp = tid >> 4;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
    if ((int64_t)blockIdx.x * 16 >= n) return;
    for (int i = tid; i < nthr; i += 256) sthr[i] = thr64[i];
    __syncthreads();
    for (int64_t b0 = (int64_t)blockIdx.x * 16; b0 < n; b0 += (int64_t)gridDim.x * 16) {
        const int64_t i = b0 + grp;
        const bool live = i < n;
        const uint64_t key = cand[live ? i : b0];
        const int64_t qi = (int64_t)(key >> 32), row = (int64_t)(key & 0xffffffffu);
        QuadQuery<T, PER> qq;
        qq.load(q + (size_t)qi * E, m);
        QuadRow<T, PER> gr;
        gr.load(gal + (size_t)row * E, m);
        const double s = quad_dot<T, PER>(qq, gr);
        if (live && m == 0 && s == s) {
            int l = 0, u = nthr;                     // bin = #{k : thresholds[k] <= s}
            while (l < u) {
                const int mid = (l + u) >> 1;
                if (sthr[mid] <= s) l = mid + 1; else u = mid;
            }
            const int cls = labels[row] == targets[qi] ? 1 : 0;
            atomicAdd(hist + ((size_t)qi * 2 + cls) * (nthr + 1) + l, 1ull);
        }
    }
}

// One workgroup per (query, class): ge[i] = rows in the bins above i (suffix sums), total = all bins
constexpr int SWEEP_FIN_PER = (MMR_SWEEP_T_MAX + 1 + 255) / 256;
__global__ __launch_bounds__(256) void sweep_finish_kernel(const unsigned long long *__restrict__ hist, int T,
                                                           const unsigned long long *__restrict__ counter, int64_t cand_cap,
                                                           int64_t *__restrict__ ge, int64_t *__restrict__ total,
                                                           int64_t *__restrict__ counts)
{
    __shared__ long long part[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r == 0 && tid == 0) {
        const unsigned long long nc = counter[0];
        counts[0] = nc < (unsigned long long)cand_cap ? (int64_t)nc : cand_cap;
        counts[1] = (int64_t)nc;
    }
    const unsigned long long *h = hist + (size_t)r * (T + 1);
    const int b0 = tid * SWEEP_FIN_PER;
    long long v[SWEEP_FIN_PER], s = 0;
#pragma unroll
    for (int j = 0; j < SWEEP_FIN_PER; ++j) {
        v[j] = b0 + j <= T ? (long long)h[b0 + j] : 0;
        s += v[j];
    }
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // inclusive suffix scan over the threads
        const long long add = tid + off < 256 ? part[tid + off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    long long run = part[tid] - s;                      // the bins of the threads above
#pragma unroll
    for (int j = SWEEP_FIN_PER - 1; j >= 0; --j) {
        const int b = b0 + j;
        run += v[j];
        if (b >= 1 && b <= T) ge[(size_t)r * T + b - 1] = run;
        if (b == 0) total[r] = run;
    }
}

struct SweepPlan {
    size_t off_cnt, off_nb, off_rb, off_qb, off_qres, off_thr, off_grid, off_hist, off_cand, off_hi, hist_bytes, total;
};

static SweepPlan make_sweep_plan(int64_t N, int E, int Q, int T, int64_t cand_cap, mmr_dtype dt, bool need_hi)
{
    SweepPlan p{};
    size_t off = 0;
    const int64_t cc = cand_cap > 0 ? cand_cap : 1;
    p.off_cnt = off; off += 256;
    p.off_nb = off; off += 256;
    p.off_rb = off; off += 256;
    const bool qsplit = dt == MMR_F32;
    p.off_qb = off; off += qsplit ? align_up((size_t)Q * E * sizeof(bf16_t), 256) : 0;
    p.off_qres = off; off += qsplit ? align_up((size_t)Q * sizeof(float), 256) : 0;
    p.off_thr = off; off += align_up((size_t)T * sizeof(double), 256);
    p.off_grid = off; off += align_up((size_t)sweep_grid_bytes(T), 256);
    p.hist_bytes = (size_t)Q * 2 * (T + 1) * sizeof(unsigned long long);
    p.off_hist = off; off += align_up(p.hist_bytes, 256);
    p.off_cand = off; off += align_up((size_t)cc * 8, 256);
    p.off_hi = off; off += (dt == MMR_F32 && need_hi) ? align_up((size_t)N * E * sizeof(bf16_t), 256) : 0;
    p.total = off;
    return p;
}

// launch_scan_kernel with a per-call LDS size: the limit is raised once to the most a call can ask for
template <auto K>
static int launch_sweep_kernel(unsigned grid, int threads, int lds, hipStream_t st, const SweepScanArgs &a)
{
    ProfScope prof(MMR_PROF_SCAN, st);
    static DeviceOnce once;
    if (once.first()) {
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, SWEEP_LDS_MAX));
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), lds, st, a);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

static int launch_sweep_scan_E(int E, const SweepScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        static_assert(C::WAVES == (decltype(e)::value <= 512 ? 8 : 4), "sweep_waves");
        const int lds = C::RING + SWEEP_LABEL_BYTES + sweep_grid_bytes(a.T) + sweep_lds_need(decltype(e)::value, a.hrows, a.T, a.stage);
        if (lds > SWEEP_LDS_MAX) { set_error("mmr_threshold_sweep: LDS plan %d > %d", lds, SWEEP_LDS_MAX); return (int)MMR_EIO; }
        if (a.row_mask) return launch_sweep_kernel<&sweep_scan_kernel<decltype(e)::value, true>>(grid, C::THREADS, lds, st, a);
        return launch_sweep_kernel<&sweep_scan_kernel<decltype(e)::value, false>>(grid, C::THREADS, lds, st, a);
    });
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_sweep_workspace_bytes(int64_t N, int E, int Q, int T, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given)
{
    if (N < 0 || Q < 0 || T < 1 || T > MMR_SWEEP_T_MAX || cand_cap < 1 || E < 1 || (dtype != MMR_F32 && dtype != MMR_BF16)) return 0;
    return make_sweep_plan(N, E, Q, T, cand_cap, dtype, !gallery_hi_given).total;
}

extern "C" int mmr_threshold_sweep(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                                   int E, const int32_t *labels, const int32_t *targets, const double *thresholds_host, int T,
                                   float gallery_norm_bound, const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                   const uint32_t *row_mask, int64_t cand_cap, int64_t *ge, int64_t *total, int64_t *counts,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_threshold_sweep";
    MMR_CHECK_ARG(dtype == MMR_F32 || dtype == MMR_BF16, "%s: dtype %d", fn, (int)dtype);
    if (!scan_supports_E(E)) { set_error("%s: E=%d unsupported (128,256,512,768)", fn, E); return MMR_ENOTSUP; }
    MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff, "%s: N=%lld outside [0, 2^31-1)", fn, (long long)N);
    MMR_CHECK_ARG(Q >= 1, "%s: Q=%d must be >= 1", fn, Q);
    MMR_CHECK_ARG(T >= 1 && T <= MMR_SWEEP_T_MAX, "%s: T=%d outside [1, %d]", fn, T, MMR_SWEEP_T_MAX);
    MMR_CHECK_ARG(thresholds_host != nullptr, "%s: null pointer (thresholds_host)", fn);
    for (int i = 0; i < T; ++i) {
        const double t = thresholds_host[i];
        MMR_CHECK_ARG(t == t && fabs(t) < INFINITY, "%s: thresholds[%d] must be finite (got %g)", fn, i, t);
        MMR_CHECK_ARG(i == 0 || thresholds_host[i - 1] < t, "%s: thresholds must be strictly ascending (thresholds[%d] = %g after %g)",
                      fn, i, t, i ? thresholds_host[i - 1] : 0.0);
    }
    MMR_CHECK_ARG(gallery_norm_bound == gallery_norm_bound && gallery_norm_bound < INFINITY, "%s: gallery_norm_bound must be finite", fn);
    MMR_CHECK_ARG(cand_cap >= 1, "%s: cand_cap=%lld must be >= 1", fn, (long long)cand_cap);
    MMR_CHECK_ARG(q != nullptr && targets != nullptr, "%s: null pointer (q / targets)", fn);
    MMR_CHECK_ARG(ge != nullptr && total != nullptr && counts != nullptr && workspace != nullptr,
                  "%s: null pointer (ge / total / counts / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr) || N == 0, "%s: null pointer (gallery / labels)", fn);
    MMR_CHECK_ARG((((uintptr_t)q | (uintptr_t)gallery | (uintptr_t)gallery_hi) & 15) == 0, "%s: q / gallery / gallery_hi must be 16-byte aligned", fn);
    MMR_CHECK_ARG((((uintptr_t)labels | (uintptr_t)targets) & 3) == 0, "%s: labels / targets must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)row_mask & 3) == 0, "%s: row_mask must be 4-byte aligned", fn);
    const bool need_hi = dtype == MMR_F32 && gallery_hi == nullptr;
    const SweepPlan p = make_sweep_plan(N, E, Q, T, cand_cap, dtype, need_hi);
    if (workspace_bytes < p.total) { set_error("%s: workspace %zu < required %zu", fn, workspace_bytes, p.total); return MMR_ENOSPC; }

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    unsigned long long *hist = (unsigned long long *)(ws + p.off_hist);
    double *thr64 = (double *)(ws + p.off_thr);
    float *grid32 = (float *)(ws + p.off_grid);
    uint64_t *cand = (uint64_t *)(ws + p.off_cand);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, 2 * sizeof(unsigned long long), st));
    MMR_CHECK_HIP(hipMemsetAsync(hist, 0, p.hist_bytes, st));
    for (int off = 0; off < T; off += SWEEP_CHUNK) {
        SweepGridChunk ch;
        const int n = T - off < SWEEP_CHUNK ? T - off : SWEEP_CHUNK;
        for (int i = 0; i < SWEEP_CHUNK; ++i) ch.t[i] = i < n ? thresholds_host[off + i] : 0.0;
        hipLaunchKernelGGL(sweep_grid_kernel, dim3(1), dim3(SWEEP_CHUNK), 0, st, ch, off, n, T, thr64, grid32);
        MMR_CHECK_LAUNCH();
    }

    if (N > 0) {
        // gallery norm bound: max(caller's, device scalar); neither -> measured here
        float host_bound = gallery_norm_bound > 0.f ? gallery_norm_bound : 0.f;
        const float *dev_bound = gallery_norm_bound_dev;
        if (host_bound == 0.f && !dev_bound) {
            float *nb = (float *)(ws + p.off_nb);
            const int rc = mmr_gallery_norm_bound(gallery, dtype, N, E, nb, stream);
            if (rc != MMR_OK) return rc;
            dev_bound = nb;
        }
        SweepScanArgs a{};
        a.gal = (const bf16_t *)gallery;
        a.resid_dev = resid_bound_dev;
        const bf16_t *qb = (const bf16_t *)q;
        if (dtype == MMR_F32) {
            if (need_hi) {
                bf16_t *hi = (bf16_t *)(ws + p.off_hi);
                float *rb = (float *)(ws + p.off_rb);
                const int rc = range_split_hi((const float *)gallery, N, E, hi, rb, st);
                if (rc != MMR_OK) return rc;
                a.gal = hi;
                a.resid_dev = rb;
            } else {
                a.gal = (const bf16_t *)gallery_hi;
            }
            bf16_t *qbw = (bf16_t *)(ws + p.off_qb);
            float *qres = (float *)(ws + p.off_qres);
            const int rc = range_queries_to_bf16((const float *)q, Q, E, qbw, qres, st);
            if (rc != MMR_OK) return rc;
            qb = qbw;
            a.qres = qres;
        }
        a.N = N;
        a.ntiles = (int)((N + RTILE - 1) / RTILE);
        a.host_bound = host_bound;
        a.dev_bound = dev_bound;
        a.split = dtype == MMR_F32;
        a.counter = counter;
        a.cand = cand;
        a.cand_cap = cand_cap;
        a.row_mask = row_mask;
        a.labels = labels;
        a.targets = targets;
        a.grid32 = grid32;
        a.T = T;
        a.hist = hist;
        a.gt0 = (float)thresholds_host[0];
        const double span = thresholds_host[T - 1] - thresholds_host[0];
        a.ginv = T > 1 ? (float)((double)(T - 1) / span) : 0.f;
        if (!(a.ginv < INFINITY) || !(fabsf(a.gt0) < INFINITY)) { a.ginv = 0.f; a.gt0 = 0.f; }   // the guess is only a guess
        // tasks as in the range scan: up to 64 tiles each, about 256 x m of them
        int tpt = 1;
        if (a.ntiles > 256) {
            const int m = (a.ntiles + 256 * RMAX_TPT - 1) / (256 * RMAX_TPT);
            tpt = (a.ntiles + 256 * m - 1) / (256 * m);
        }
        a.tpt = tpt;
        const int ntasks = (a.ntiles + tpt - 1) / tpt;
        const int qpp = sweep_queries_per_pass(E, T);
        a.hrows = Q < qpp ? Q : qpp;
        a.stage = sweep_stage_entries(E, T, a.hrows);
        for (int q0 = 0; q0 < Q; q0 += qpp) {
            a.q0 = q0;
            a.Qc = (Q - q0) < qpp ? (Q - q0) : qpp;
            a.ncw = (a.Qc + 31) / 32;
            a.q = qb + (size_t)q0 * E;
            const int rc = launch_sweep_scan_E(E, a, (unsigned)ntasks, st);
            if (rc != MMR_OK) return rc;
        }
        ProfScope prof(MMR_PROF_FINALIZE, st);
        const int64_t rb = (cand_cap + 15) / 16;
        const dim3 grid((unsigned)(rb < 8192 ? rb : 8192));
        if (dtype == MMR_BF16) {
            MMR_DISPATCH_PER(E, {
                hipLaunchKernelGGL((sweep_recheck_kernel<bf16_t, PER>), grid, dim3(256), T * sizeof(double), st, (const bf16_t *)q,
                                   (const bf16_t *)gallery, labels, targets, (const double *)thr64, T,
                                   (const unsigned long long *)counter, (const uint64_t *)cand, cand_cap, hist);
            });
        } else {
            MMR_DISPATCH_PER(E, {
                hipLaunchKernelGGL((sweep_recheck_kernel<float, PER>), grid, dim3(256), T * sizeof(double), st, (const float *)q,
                                   (const float *)gallery, labels, targets, (const double *)thr64, T,
                                   (const unsigned long long *)counter, (const uint64_t *)cand, cand_cap, hist);
            });
        }
        MMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sweep_finish_kernel, dim3((unsigned)(2 * Q)), dim3(256), 0, st, (const unsigned long long *)hist, T,
                       (const unsigned long long *)counter, cand_cap, ge, total, counts);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
