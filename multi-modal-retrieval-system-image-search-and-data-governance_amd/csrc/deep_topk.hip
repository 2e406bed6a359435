// Exact top-k for k up to MMR_DEEP_K_MAX (4096) on gfx950 (MI355X): a per-query threshold taken from the bucket maxima
// of the ordinary top-k scan replaces the fixed KS_MAX candidate tiles of mmr_cosine_topk.
//
// Structure ("deep top-k"):
//   pass A                  the top-k scan of search.hip, unchanged (topk_scan.h): bmax[tile][q] = maximum of the approximate
//                           (fp32 MFMA) dots over the tile's live, non-NaN rows; -inf for a dead tile.
//   deep_hist_kernel /      per query the exact k-th largest b_k of its bmax column (MSB radix select over order-preserving
//   deep_select_kernel      uint32 keys, LDS histograms per slab of tiles), ||q|| in fp64 and scan_margin's eps
//                           (range_common.h) -> thr_acc = b_k - 2 eps (fp32, rounded down), thr_exact = b_k - eps (fp64,
//                           rounded down).
//   deep_list_kernel        the (query, tile) pairs with bmax >= thr_acc, compacted per workgroup, one atomic each.
//   deep_rescore_kernel     one wave per listed pair: exact fp64 dots (quad_dot, the order oracle/search_ref.c replicates) of
//                           the tile's live rows on the ORIGINAL rows; keeps dot64 >= thr_exact.
//   rocPRIM radix sorts     survivors by (query, row), then stably by the descending image of dot64, then stably by query:
//                           (query, -dot64, +row) order.  deep_emit_kernel writes the first k of every query.
// Why this is exact: |acc - dot64| <= eps for every live non-NaN row of a query that is not `wild`.  The k tiles whose
// maxima reach b_k each hold a row with dot64 >= b_k - eps, so the k-th best exact dot d_k >= b_k - eps; every top-k row
// then has acc >= b_k - 2 eps and sits in a listed tile, and it survives the exact cut.  Wild queries (scan_margin) and
// queries with fewer than k tiles get -inf thresholds: every tile is listed and every non-NaN row survives.
// Integer atomics only: the lists' orders depend on arrival, the sorted output and the counts do not.
#include "mmr_common.h"
#include "exact_dot.h"
#include "range_common.h"
#include "scan_pipeline.h"
#include "topk_scan.h"
#include "scan_host.h"
#include "radix_sort_host.h"
#include "row_lists.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

constexpr int DT_QB = 32;                        // queries per threshold workgroup: one 128-byte line of a bmax row
constexpr int DT_THREADS = 1024;
constexpr int DT_RG = DT_THREADS / DT_QB;        // tiles a workgroup reads per step
constexpr int DT_UNROLL = 4;                     // bmax loads in flight per thread
constexpr int DT_BINS = 256 * DT_QB;             // one histogram: [digit][query of the block]
constexpr int DT_SLAB_TILES = 256;               // a slab holds at least this many tiles ...
constexpr int DT_SLAB_MAX = 64;                  // ... and a query block is cut into at most this many slabs

// The k-th largest of every bmax column: an MSB radix select over order-preserving uint32 keys, four passes of 8 bits.
// One workgroup reading a whole column block is latency-bound (31 250 tiles at 1M rows), so a pass is two launches: deep_hist_kernel, grid (query blocks, slabs), counts the digits of the keys that match the prefix found
// so far over its slab of tiles in an LDS histogram hist[digit][query] and stores it; deep_select_kernel adds the slabs
// and finds per query the bin that holds the need-th largest key.
// Thread (qi = tid & 31, rg = tid >> 5) reads bmax[t][col0 + qi] for t = rg, rg + 32, ...: a half-wave reads one line, and
// its LDS atomics hit 32 different banks.
__global__ __launch_bounds__(DT_THREADS) void deep_hist_kernel(const float *__restrict__ bmax, int ntiles, int qpad, int pass,
                                                               int tiles_per_slab, const uint32_t *__restrict__ sel_prefix,
                                                               uint32_t *__restrict__ slab_hist)
{
    __shared__ uint32_t hist[DT_BINS];
    const int tid = threadIdx.x, qi = tid & (DT_QB - 1), rg = tid >> 5;
    const int col = blockIdx.x * DT_QB + qi;                 // < qpad: qpad is a multiple of 32
    for (int i = tid; i < DT_BINS; i += DT_THREADS) hist[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass ? 0xffffffffu << (shift + 8) : 0u;
    const uint32_t pfx = pass ? sel_prefix[col] : 0u;
    const int t1 = min(ntiles, ((int)blockIdx.y + 1) * tiles_per_slab);
    const float *p = bmax + col;
    int t = blockIdx.y * tiles_per_slab + rg;
    for (; t + (DT_UNROLL - 1) * DT_RG < t1; t += DT_UNROLL * DT_RG) {
        float v[DT_UNROLL];
#pragma unroll
        for (int u = 0; u < DT_UNROLL; ++u) v[u] = p[(size_t)(t + u * DT_RG) * qpad];
#pragma unroll
        for (int u = 0; u < DT_UNROLL; ++u) {
            const uint32_t key = ord_f32(v[u]);
            if ((key & himask) == pfx) atomicAdd(&hist[((key >> shift) & 255u) * DT_QB + qi], 1u);
        }
    }
    for (; t < t1; t += DT_RG) {
        const uint32_t key = ord_f32(p[(size_t)t * qpad]);
        if ((key & himask) == pfx) atomicAdd(&hist[((key >> shift) & 255u) * DT_QB + qi], 1u);
    }
    __syncthreads();
    uint32_t *out = slab_hist + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * DT_BINS;
    for (int i = tid; i < DT_BINS; i += DT_THREADS) out[i] = hist[i];
}

// Selection step of one pass.  A workgroup owns DS_QW = 4 queries of a block (grid: query blocks x 8): thread (digit,
// query) adds that bin over the slabs -- independent loads, eight in flight -- then the 32 lanes of half-wave `query` own 8 bins each and find the bin that holds the need-th
// largest key by a suffix sum over shuffles.  sel_prefix / sel_need / sel_short carry the state between the passes.  The
// last pass also sums the squares of the query the scan multiplied in fp64, calls scan_margin and writes the thresholds.
// SQ: element type of the scan's queries (bf16, or fp32 for scan_f32s_kernel).
constexpr int DS_QW = 4;
constexpr int DS_PARTS = DT_QB / DS_QW;
static_assert(256 * DS_QW == DT_THREADS, "one thread per (digit, query) bin");

template <typename SQ>
__global__ __launch_bounds__(DT_THREADS) void deep_select_kernel(
    const uint32_t *__restrict__ slab_hist, int nslab, int pass, int Qc, int q0, int k, uint32_t *__restrict__ sel_prefix,
    uint32_t *__restrict__ sel_need, uint32_t *__restrict__ sel_short, const SQ *__restrict__ sq, int E, float host_bound,
    const float *__restrict__ dev_bound, int split, const float *__restrict__ resid_dev, const float *__restrict__ qres,
    float *__restrict__ thr_acc, double *__restrict__ thr_exact)
{
    __shared__ uint32_t hist[256 * DS_QW];                   // [digit][query of this workgroup]
    const int tid = threadIdx.x;
    {
        const uint32_t *in = slab_hist + (size_t)blockIdx.x * nslab * DT_BINS + (tid >> 2) * DT_QB + blockIdx.y * DS_QW + (tid & 3);
        uint32_t sum = 0;
        int sl = 0;
        for (; sl + 8 <= nslab; sl += 8) {
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = in[(size_t)(sl + u) * DT_BINS];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        for (; sl < nslab; ++sl) sum += in[(size_t)sl * DT_BINS];
        hist[tid] = sum;
    }
    __syncthreads();
    if (tid >= DS_QW * 32) return;                           // two waves go on: nothing below crosses a half-wave
    const int query = tid >> 5, j = tid & 31;                // half-wave `query`, bins [8j, 8j + 8)
    const int col = blockIdx.x * DT_QB + blockIdx.y * DS_QW + query;
    const int shift = 24 - 8 * pass;
    uint32_t c[8], s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { c[i] = hist[(8 * j + i) * DS_QW + query]; s += c[i]; }
    uint32_t incl = s;                                       // keys in the bins of lanes >= j of this half-wave
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const uint32_t v = __shfl_down(incl, off, 32);
        incl += j + off < 32 ? v : 0u;
    }
    uint32_t above = incl - s;
    const uint32_t need = pass ? sel_need[col] : (uint32_t)k;
    const uint32_t pfx = pass ? sel_prefix[col] : 0u;
    const uint32_t total = __shfl(incl, 0, 32);
    if (pass == 0 && j == 0) {
        sel_short[col] = total < need;                       // fewer than k tiles: b_k = -inf
        if (total < need) { sel_prefix[col] = 0; sel_need[col] = need; }
    }
    uint32_t found = 0;                                      // the digit this pass adds to the prefix, in the lane that holds it
    if (above < need && need <= above + s) {
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            if (above < need && need <= above + c[i]) {
                found = (uint32_t)(8 * j + i) << shift;
                sel_prefix[col] = pfx | found;
                sel_need[col] = need - above;
            }
            above += c[i];
        }
    }
    if (pass < 3) return;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) found |= __shfl_xor(found, off, 32);
    const int lq = col;                                      // query of this chunk
    if (lq >= Qc) return;                                    // whole half-waves leave: the shuffles below stay inside one
    double ss = 0.0;                                         // fp64, fixed order: a small query's squares underflow in fp32
    for (int e = j; e < E; e += 32) {
        double x;
        if constexpr (__is_same(SQ, bf16_t)) x = bf16_to_f32(sq[(size_t)lq * E + e]);
        else x = (float)sq[(size_t)lq * E + e];      // fp16 and fp32: exact
        ss += x * x;
    }
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 32);
    if (j == 0) {
        const int64_t gq = (int64_t)q0 + lq;
        const ScanMargin mg = scan_margin(ss, host_bound, dev_bound, split, resid_dev, qres, gq);
        const float bk = unord_f32(pfx | found);
        float ta = -INFINITY;
        double te = -INFINITY;
        if (!mg.wild && !sel_short[col] && fabsf(bk) < INFINITY) {
            // both rounded towards -inf: a threshold that is too low only lists more
            te = nextafter((double)bk - mg.eps, -INFINITY);
            const double lo = nextafter((double)bk - 2.0 * mg.eps, -INFINITY);
            ta = (float)lo;
            if ((double)ta > lo) ta = nextafterf(ta, -INFINITY);
        }
        thr_acc[gq] = ta;
        thr_exact[gq] = te;
    }
}

// (query, tile) pairs of this chunk with bmax >= thr_acc: appended as (query << 32) | tile.  A workgroup takes whole tiles,
// about 2048 (tile, query) entries at a time, compacts its hits over the workgroup and appends them with ONE atomic (atomics
// on the one counter serialise, so there are few of them).  counter[0] keeps counting past the
// capacity, the stores stop at it.
constexpr int DL_PER = 8;
__global__ __launch_bounds__(256) void deep_list_kernel(const float *__restrict__ bmax, int ntiles, int qpad, int Qc, int q0,
                                                        const float *__restrict__ thr_acc, unsigned long long *__restrict__ counter,
                                                        uint64_t *__restrict__ tiles, int64_t tile_cap)
{
    __shared__ int s_wave[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = 256 * DL_PER / qpad;                      // tiles per step: qpad <= 256
    for (int64_t t0 = (int64_t)blockIdx.x * tb; t0 < ntiles; t0 += (int64_t)gridDim.x * tb) {
        const int nel = (int)(ntiles - t0 < tb ? ntiles - t0 : tb) * qpad;
        const float *p = bmax + (size_t)t0 * qpad;
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < DL_PER; ++i) {
            const int l = i * 256 + tid;
            const int c = l % qpad;
            const bool in = l < nel && c < Qc;
            if (in && p[l] >= thr_acc[q0 + c]) bits |= 1u << i;
        }
        const WavePrefix wp = wave_prefix(__popc(bits), lane);
        if (lane == 0) s_wave[wave] = wp.total;
        __syncthreads();
        int before = wp.before, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { before += w < wave ? s_wave[w] : 0; total += s_wave[w]; }
        if (tid == 0 && total > 0) s_base = atomicAdd(counter, (unsigned long long)total);
        __syncthreads();
        if (total > 0) {
            unsigned long long pos = s_base + (unsigned long long)before;
#pragma unroll
            for (int i = 0; i < DL_PER; ++i) {
                if (bits & (1u << i)) {
                    const int l = i * 256 + tid;
                    if (pos < (unsigned long long)tile_cap)
                        tiles[pos] = ((uint64_t)(q0 + l % qpad) << 32) | (uint64_t)(t0 + l / qpad);
                    ++pos;
                }
            }
        }
    }
}

// deep_rescore_kernel: one wave per listed pair, exact fp64 dots of the tile's live rows.  Its body is deep_rescore_body.inc,
// shared with the per-query-mask form (deep_qmask.hip).
template <typename T, int PER>
__global__ __launch_bounds__(256) void deep_rescore_kernel(const T *__restrict__ q, const T *__restrict__ gal, int64_t N,
                                                           int tile_rows, const uint32_t *__restrict__ row_mask,
                                                           unsigned long long *__restrict__ counter,
                                                           const uint64_t *__restrict__ tiles, int64_t tile_cap,
                                                           const double *__restrict__ thr_exact, uint64_t *__restrict__ surv_k,
                                                           uint64_t *__restrict__ surv_o, int64_t surv_cap)
{
    constexpr bool QM = false;
    constexpr const uint32_t *row_masks = nullptr;
    constexpr int64_t mask_stride = 0;
#include "deep_rescore_body.inc"
}

// One workgroup per query: its survivors are the run of keys with this query id in the sorted list, best first.
// Writes int64 ids; slots past the run hold -1 / -inf / -inf.
__global__ __launch_bounds__(256) void deep_emit_kernel(const unsigned long long *__restrict__ counter,
                                                        const uint64_t *__restrict__ sk, const uint64_t *__restrict__ so,
                                                        int64_t surv_cap, int k, float scale, int64_t *__restrict__ idx,
                                                        float *__restrict__ score, double *__restrict__ dot64,
                                                        int64_t *__restrict__ counts)
{
    const uint64_t q = blockIdx.x;
    if (q == 0 && threadIdx.x == 0) {
        counts[0] = (int64_t)counter[0];
        counts[1] = (int64_t)counter[1];
    }
    const unsigned long long ns = counter[1];
    const int64_t n = ns < (unsigned long long)surv_cap ? (int64_t)ns : surv_cap;
    int64_t lo = 0, hi = n;                          // first entry of query q
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((sk[mid] >> 32) < q) lo = mid + 1; else hi = mid;
    }
    for (int j = threadIdx.x; j < k; j += 256) {
        const int64_t p = lo + j;
        const bool ok = p < n && (sk[p < n ? p : 0] >> 32) == q;
        const double d = ok ? unord_f64(~so[p]) : -INFINITY;
        const size_t o = (size_t)q * k + j;
        idx[o] = ok ? (int64_t)(sk[p] & 0xffffffffu) : -1;
        score[o] = ok ? (float)(d * (double)scale) : -INFINITY;
        if (dot64) dot64[o] = d;
    }
}

struct DeepPlan {
    TopkScanGeom geom;
    mmr_dtype scan_dtype;       // operands of pass A
    bool split;                 // fp32 gallery scanned through the caller's bf16 hi half
    int nslab, tiles_per_slab;  // threshold select: slabs of tiles per query block
    size_t off_cnt, off_nb, off_qb, off_qres, off_thra, off_thre, off_sel, off_slab, off_bmax, off_tmax, off_tiles, off_sk, off_so, off_sk2,
        off_so2, off_tmp, tmp_bytes, total;
};

// qmasked: the plan of mmr_cosine_topk_deep_qmasked -- 16-bit scan operands only, and tasks short enough for their mask
// words to sit in LDS (qmask_scan_tpt), so tmax has more rows
static DeepPlan make_deep_plan(int64_t N, int E, int Q, int64_t tile_cap, int64_t surv_cap, mmr_dtype dt, bool split_given,
                               bool qmasked = false)
{
    DeepPlan p{};
    p.split = dt == MMR_F32 && split_given;
    p.scan_dtype = p.split ? MMR_BF16 : dt;
    p.geom = topk_scan_geom(N, E, p.scan_dtype);
    const size_t Q1 = Q > 0 ? Q : 1;
    const int qc = Q < p.geom.qmax ? (Q + 31) / 32 * 32 : p.geom.qmax;
    if (qmasked && p.geom.ntiles > 0) {
        p.geom.tpt = qmask_scan_tpt(E, qc, p.geom.tpt);
        p.geom.ntasks = (p.geom.ntiles + p.geom.tpt - 1) / p.geom.tpt;
    }
    const size_t tc = tile_cap > 0 ? tile_cap : 1, sc = surv_cap > 0 ? surv_cap : 1;
    WsLayout l;
    p.off_cnt = l.take(2 * sizeof(unsigned long long));
    p.off_nb = l.take(sizeof(float));
    p.off_qb = l.take(p.split ? Q1 * E * sizeof(bf16_t) : 0);
    p.off_qres = l.take(p.split ? Q1 * sizeof(float) : 0);
    p.off_thra = l.take(Q1 * sizeof(float));
    p.off_thre = l.take(Q1 * sizeof(double));
    p.nslab = (p.geom.ntiles + DT_SLAB_TILES - 1) / DT_SLAB_TILES;
    p.nslab = p.nslab < 1 ? 1 : (p.nslab > DT_SLAB_MAX ? DT_SLAB_MAX : p.nslab);
    p.tiles_per_slab = (p.geom.ntiles + p.nslab - 1) / p.nslab;
    p.off_sel = l.take((size_t)3 * qc * sizeof(uint32_t));
    p.off_slab = l.take((size_t)(qc / DT_QB) * p.nslab * DT_BINS * sizeof(uint32_t));
    p.off_bmax = l.take((size_t)p.geom.ntiles * qc * sizeof(float));
    p.off_tmax = l.take((size_t)p.geom.ntasks * qc * sizeof(float));
    p.off_tiles = l.take(tc * 8);
    p.off_sk = l.take(sc * 8);
    p.off_so = l.take(sc * 8);
    p.off_sk2 = l.take(sc * 8);
    p.off_so2 = l.take(sc * 8);
    p.tmp_bytes = sort_bytes<uint64_t>((int64_t)sc);
    p.off_tmp = l.take(p.tmp_bytes > 0 ? p.tmp_bytes : 1);
    p.total = l.off;
    return p;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_deep_topk_workspace_bytes(int64_t N, int E, int Q, int k, int64_t tile_cap, int64_t surv_cap,
                                                mmr_dtype dtype, int split_given)
{
    if (N < 0 || N >= 0x7fffffff || Q < 0 || k < 1 || k > MMR_DEEP_K_MAX || tile_cap < 1 || surv_cap < 1 || !scan_supports_E(E) ||
        (dtype != MMR_F32 && dtype != MMR_BF16 && dtype != MMR_F16))
        return 0;
    return make_deep_plan(N, E, Q, tile_cap, surv_cap, dtype, split_given != 0).total;
}

extern "C" size_t mmr_deep_topk_qmasked_workspace_bytes(int64_t N, int E, int Q, int k, int64_t tile_cap, int64_t surv_cap,
                                                        mmr_dtype dtype, int split_given)
{
    if (N < 0 || N >= 0x7fffffff || Q < 0 || k < 1 || k > MMR_DEEP_K_MAX || tile_cap < 1 || surv_cap < 1 || !scan_supports_E(E) ||
        (dtype != MMR_F32 && dtype != MMR_BF16 && dtype != MMR_F16) || (dtype == MMR_F32 && !split_given))
        return 0;
    return make_deep_plan(N, E, Q, tile_cap, surv_cap, dtype, split_given != 0, true).total;
}

// mmr_cosine_topk_deep (qmasked = false: row_masks / mask_stride unused) and mmr_cosine_topk_deep_qmasked
static int deep_impl(const char *fn, bool qmasked, const void *q, const void *gallery, const void *gallery_hi,
                     const float *split_resid_bound_dev, mmr_dtype dtype, int Q, int64_t N, int E, int k, float scale,
                     float gallery_norm_bound, const float *gallery_norm_bound_dev, const uint32_t *row_masks, int64_t mask_stride,
                     const uint32_t *row_mask, int64_t tile_cap, int64_t surv_cap, int64_t *idx, float *score, double *dot64,
                     int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.sizes_int32(Q, N));
    MMR_CHECK_ARG(k >= 1 && k <= MMR_DEEP_K_MAX, "%s: k=%d outside [1,%d]", fn, k, MMR_DEEP_K_MAX);
    MMR_TRY(ck.scale_finite(scale));
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_TRY(ck.scan_E(E));
    if (Q == 0) return MMR_OK;
    MMR_CHECK_ARG(tile_cap >= 1 && surv_cap >= 1, "%s: tile_cap=%lld and surv_cap=%lld must be >= 1", fn, (long long)tile_cap,
                  (long long)surv_cap);
    MMR_CHECK_ARG(q && idx && score && counts && (gallery || N == 0), "%s: null pointer", fn);
    MMR_TRY(ck.aligned16((uintptr_t)q | (uintptr_t)gallery | (uintptr_t)gallery_hi, "q / gallery / gallery_hi"));
    MMR_TRY(ck.row_mask(row_mask));
    if (qmasked) {
        MMR_CHECK_ARG(row_masks != nullptr || N == 0, "%s: null pointer (row_masks)", fn);
        MMR_CHECK_ARG(((uintptr_t)row_masks & 3) == 0, "%s: row_masks must be 4-byte aligned", fn);
        MMR_CHECK_ARG(mask_stride >= (N + 31) / 32, "%s: mask_stride=%lld below ceil(N/32)=%lld words", fn, (long long)mask_stride,
                      (long long)((N + 31) / 32));
        MMR_CHECK_ARG(dtype != MMR_F32 || gallery_hi != nullptr,
                      "%s: an fp32 gallery needs gallery_hi (mmr_gallery_split_bf16): the fp32 row scan has no row_masks form", fn);
    }
    MMR_CHECK_ARG(workspace != nullptr, "%s: null workspace", fn);
    const DeepPlan p = make_deep_plan(N, E, Q, tile_cap, surv_cap, dtype, gallery_hi != nullptr, qmasked);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));
    if (p.tmp_bytes == 0) { set_error("%s: sort storage query failed", fn); return MMR_EIO; }

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    float *thr_acc = (float *)(ws + p.off_thra);
    double *thr_exact = (double *)(ws + p.off_thre);
    uint64_t *tiles = (uint64_t *)(ws + p.off_tiles);
    uint64_t *sk = (uint64_t *)(ws + p.off_sk), *so = (uint64_t *)(ws + p.off_so);
    uint64_t *sk2 = (uint64_t *)(ws + p.off_sk2), *so2 = (uint64_t *)(ws + p.off_so2);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, 2 * sizeof(unsigned long long), st));
    // sort padding: keys above every real key (Q << 32 for the (query, row) keys, ~0 for the dot keys), so they sort last
    MMR_TRY(fill_u64(sk, surv_cap, (uint64_t)Q << 32, st));
    // Q == 1: no third sort, so the padding must sort last by its dot key (a survivor's key is never ~0: the image of a NaN)
    if (Q == 1) MMR_TRY(fill_u64(so, surv_cap, ~(uint64_t)0, st));

    if (N > 0) {
        const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, gallery_norm_bound_dev, (float *)(ws + p.off_nb), st);
        MMR_TRY(nb.rc);
        ScanOperands ops;       // split: bf16-rounded queries over the caller's hi half; else the caller's arrays
        MMR_TRY(scan_operands(p.split, q, Q, gallery, gallery_hi, split_resid_bound_dev, N, E, nullptr, nullptr,
                              (bf16_t *)(ws + p.off_qb), (float *)(ws + p.off_qres), st, &ops));
        const size_t sesz = p.scan_dtype == MMR_F32 ? 4 : 2;
        float *bmax = (float *)(ws + p.off_bmax), *tmax = (float *)(ws + p.off_tmax);
        for (int q0 = 0; q0 < Q; q0 += p.geom.qmax) {
            const int Qc = (Q - q0) < p.geom.qmax ? (Q - q0) : p.geom.qmax;
            const int qpad = (Qc + 31) / 32 * 32;
            const char *qc = (const char *)ops.q + (size_t)q0 * E * sesz;
            if (qmasked)
                MMR_TRY(launch_topk_scan_qmasked(p.scan_dtype, E, qc, ops.gal, Qc, N, p.geom.ntiles, p.geom.tpt, qpad, bmax, tmax,
                                                 row_masks + (size_t)q0 * mask_stride, mask_stride, row_mask, st));
            else MMR_TRY(launch_topk_scan(p.scan_dtype, E, qc, ops.gal, Qc, N, p.geom, qpad, bmax, tmax, row_mask, st));
            ProfScope prof(MMR_PROF_FINALIZE, st);
            uint32_t *sel_prefix = (uint32_t *)(ws + p.off_sel), *sel_need = sel_prefix + qpad, *sel_short = sel_need + qpad;
            uint32_t *slab_hist = (uint32_t *)(ws + p.off_slab);
            for (int pass = 0; pass < 4; ++pass) {
                hipLaunchKernelGGL(deep_hist_kernel, dim3(qpad / DT_QB, p.nslab), dim3(DT_THREADS), 0, st, (const float *)bmax,
                                   p.geom.ntiles, qpad, pass, p.tiles_per_slab, (const uint32_t *)sel_prefix, slab_hist);
                MMR_CHECK_LAUNCH();
                dispatch_elem(p.scan_dtype, [&](auto tag) -> int {
                    using T = typename decltype(tag)::type;
                    hipLaunchKernelGGL(deep_select_kernel<T>, dim3(qpad / DT_QB, DS_PARTS), dim3(DT_THREADS), 0, st,
                                       (const uint32_t *)slab_hist, p.nslab, pass, Qc, q0, k, sel_prefix, sel_need, sel_short,
                                       (const T *)qc, E, nb.host, nb.dev, (int)p.split, ops.resid, ops.qres, thr_acc, thr_exact);
                    return MMR_OK;
                });
                MMR_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(deep_list_kernel, dim3(grid_1d(p.geom.ntiles, 256 * DL_PER / qpad, 2048)), dim3(256), 0, st, (const float *)bmax,
                               p.geom.ntiles, qpad, Qc, q0, (const float *)thr_acc, counter, tiles, tile_cap);
            MMR_CHECK_LAUNCH();
        }
        {
            ProfScope prof(MMR_PROF_EXACT, st);
            if (qmasked)
                MMR_TRY(launch_deep_rescore_qmasked(dtype, E, q, gallery, N, p.geom.tile_rows, row_mask, row_masks, mask_stride, counter,
                                                    tiles, tile_cap, thr_exact, sk, so, surv_cap, st));
            else scan_dispatch_E(E, [&](auto e) {       // E passed scan_supports_E: no E = 1024 variant is built
                return dispatch_elem(dtype, [&](auto tag) -> int {
                    using T = typename decltype(tag)::type;
                    const dim3 grid(grid_1d(tile_cap, 4, 8192));
                    hipLaunchKernelGGL((deep_rescore_kernel<T, decltype(e)::value / 64>), grid, dim3(256), 0, st, (const T *)q,
                                       (const T *)gallery, N, p.geom.tile_rows, row_mask, counter, (const uint64_t *)tiles, tile_cap,
                                       (const double *)thr_exact, sk, so, surv_cap);
                    return MMR_OK;
                });
            });
            MMR_CHECK_LAUNCH();
        }
    }

    ProfScope prof(MMR_PROF_FINALIZE, st);
    const uint64_t *fk = sk, *fo = so;              // N == 0: nothing to sort, the emit kernel sees no survivors
    if (N > 0) {
        // (query, row) order, then stably by descending dot64, then (more than one query) stably by query:
        // (query, -dot64, +row).  The padding (query id Q) sorts last in the first and the third sort; with one query the
        // second sort is the last and the padding's dot keys (~0) put it last there.
        const int qbits = bitlen64((uint64_t)Q);
        void *tmp = ws + p.off_tmp;
        MMR_TRY(sort_pairs(fn, tmp, p.tmp_bytes, sk, sk2, so, so2, surv_cap, 0, 32 + qbits, st));
        MMR_TRY(sort_pairs(fn, tmp, p.tmp_bytes, so2, so, sk2, sk, surv_cap, 0, 64, st));
        fk = sk;
        fo = so;
        if (Q > 1) {
            MMR_TRY(sort_pairs(fn, tmp, p.tmp_bytes, sk, sk2, so, so2, surv_cap, 32, 32 + qbits, st));
            fk = sk2;
            fo = so2;
        }
    }
    hipLaunchKernelGGL(deep_emit_kernel, dim3(Q), dim3(256), 0, st, (const unsigned long long *)counter, fk, fo, surv_cap, k,
                       scale, idx, score, dot64, counts);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_cosine_topk_deep(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                    const float *split_resid_bound_dev, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                                    float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                                    const uint32_t *row_mask, int64_t tile_cap, int64_t surv_cap, int64_t *idx, float *score,
                                    double *dot64, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)gallery_lo;      // pass A scans the hi half alone; the lo half is accepted so that a split index passes what it holds
    return deep_impl("mmr_cosine_topk_deep", false, q, gallery, gallery_hi, split_resid_bound_dev, dtype, Q, N, E, k, scale,
                     gallery_norm_bound, gallery_norm_bound_dev, nullptr, 0, row_mask, tile_cap, surv_cap, idx, score, dot64, counts,
                     workspace, workspace_bytes, stream);
}

extern "C" int mmr_cosine_topk_deep_qmasked(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                            const float *split_resid_bound_dev, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                                            float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                                            const uint32_t *row_masks, int64_t mask_stride, const uint32_t *row_mask,
                                            int64_t tile_cap, int64_t surv_cap, int64_t *idx, float *score, double *dot64,
                                            int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)gallery_lo;
    return deep_impl("mmr_cosine_topk_deep_qmasked", true, q, gallery, gallery_hi, split_resid_bound_dev, dtype, Q, N, E, k, scale,
                     gallery_norm_bound, gallery_norm_bound_dev, row_masks, mask_stride, row_mask, tile_cap, surv_cap, idx, score,
                     dot64, counts, workspace, workspace_bytes, stream);
}
