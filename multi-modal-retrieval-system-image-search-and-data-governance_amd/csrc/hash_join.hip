// Perceptual-hash Hamming joins for gfx950 (MI355X): the duplicate rule of the reference's clean-up tools on the device.
//
// Replaces the two O(N^2) hash loops of the reference
//     are_images_similar: phash / dhash / whash, ANY distance <= 5        reference tool/find_repeated_in_same_folder.py:38-54, :76-95
//     train image dropped when a test dhash lies within the threshold   reference tool/delete repeated.py:11,120-135
// with one launch over a tile grid.  A row is H hashes of W 64-bit words; a pair matches iff for some enabled kind h
// popcount(a[h] ^ b[h]) <= thr[h].  Everything is integer-exact: XOR, population count, compare -- no margin, no recheck.
//
// Structure ("hash join"):
//   hash_join_kernel<H, W, SELF>   a workgroup takes HJ_TILE x HJ_TILE tiles from a linearised list (SELF: the tiles on or
//                                  above the diagonal only).  Each lane holds HJ_CPL "column" rows in VGPRs for the whole
//                                  tile; the tile's "row" rows are wave-uniform and arrive through the scalar path (SGPR
//                                  operands of v_xor), RU rows per step, the next step's loaded while this one computes
//                                  (HashCfg: while two steps fit 32 SGPRs).
//                                  Per step every lane reduces min over its pairs and kinds of (distance - thr); only a
//                                  wave in which some lane reaches <= 0 enters the append path, which is where rows and
//                                  columns are excluded BY INDEX (past the end, masked, i >= j) -- never by a pad value.
//                                  Matches are compacted per wave (wave_prefix) and appended with one 64-bit atomicAdd
//                                  per wave and step; the counter keeps counting past `cap`, the stores stop at it.
//   rocPRIM radix sort             the appended (key = first << 32 | second, packed distances) by key: the append order is
//                                  arbitrary, the output is not.
//   hash_emit_kernel               the sorted pairs to the caller's arrays, and counts[0].
#include "mmr_common.h"
#include "range_common.h"
#include "radix_sort_host.h"

#include <hip/hip_runtime.h>

namespace mmr {

constexpr int HJ_THREADS = 256;
constexpr int HJ_CPL = 4;                          // column rows per lane
constexpr int HJ_TILE = HJ_THREADS * HJ_CPL;       // rows and columns per tile (tests/test_hash_join_gpu.py names it)
constexpr int HJ_OFF = 1 << 20;                    // bias of a disabled kind: distance + HJ_OFF is never <= 0
constexpr int64_t HJ_MAX_GRID = 1 << 20;           // workgroups per launch; a larger tile list is strided over

// RU: rows of the uniform side per step
template <int H, int W>
struct HashCfg {
    static constexpr int HW = H * W;
    static constexpr int RU = HW <= 2 ? 4 : (HW <= 4 ? 2 : 1);
    // the next step's rows are loaded while this one computes, up to 8 words a step (32 SGPRs for the two steps); a longer
    // row has some hundred VALU instructions per step to cover its load behind the SIMD's other waves
    static constexpr bool PREFETCH = RU * HW <= 8;
};

struct HashBias {
    int v[4];       // -thr[h] for an enabled kind, HJ_OFF for a disabled or absent one
};

// distance of kind h as the append path computes it, for the packed distances of a stored pair: through
// popcount(a ^ b) = popcount(a | b) - popcount(a & b), so that it shares no instruction with the hot loop.
// Written as the hot loop writes it, the compiler merges the two and keeps every partial sum of a step alive in VGPRs
// across the branch (H = 4, W = 4: past the register file, into scratch).
template <int W>
__device__ __forceinline__ int hash_dist_cold(const uint64_t *a, const uint64_t *b, int h)
{
    int d = 0;
#pragma unroll
    for (int w = 0; w < W; ++w)
        d += __popcll(a[h * W + w] | b[h * W + w]) - __popcll(a[h * W + w] & b[h * W + w]);
    return d;
}

// distance of kind h, plus `start`
template <int W>
__device__ __forceinline__ int hash_dist(const uint64_t *a, const uint64_t *b, int h, int start)
{
    int e = start;      // each half-word is one v_bcnt_u32_b32 that adds to the running sum
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t x = a[h * W + w] ^ b[h * W + w];
        e = __popc((uint32_t)x) + e;
        e = __popc((uint32_t)(x >> 32)) + e;
    }
    return e;
}

// rows [nrows, H, W]: the wave-uniform side (SELF: also the columns); cols [ncols, H, W]: the lanes' side.  row_mask covers
// the columns, and in the self-join the rows too.  lists: the match counter, then (256 bytes on) the keys (row << 32) | column
// and behind them the packed distances, `cap` (rounded up to 32) of each -- one pointer, to spare the hot loop SGPRs.
template <int H, int W, bool SELF>
__global__ __launch_bounds__(HJ_THREADS) void hash_join_kernel(const uint64_t *__restrict__ rows, const uint64_t *__restrict__ cols,
                                                               int nrows, int ncols, int ntc, int64_t ntiles, HashBias bias,
                                                               const uint32_t *__restrict__ row_mask,
                                                               unsigned long long *__restrict__ lists, int64_t cap)
{
    constexpr int HW = HashCfg<H, W>::HW, RU = HashCfg<H, W>::RU;
    constexpr bool PREFETCH = HashCfg<H, W>::PREFETCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t *__restrict__ cside = SELF ? rows : cols;

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t tr, tc;
        if (SELF) {
            // t = tc (tc + 1) / 2 + tr, tr <= tc: the upper triangle, column by column (8 t + 1 < 2^53 for N < 2^31)
            tc = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
            while (tc * (tc + 1) / 2 > t) --tc;
            while ((tc + 1) * (tc + 2) / 2 <= t) ++tc;
            tr = t - tc * (tc + 1) / 2;
        } else {
            tr = t / ntc;
            tc = t - tr * ntc;
        }
        const int r0 = (int)tr * HJ_TILE, c0 = (int)tc * HJ_TILE;        // ids are below 2^31
        const int rcount = nrows - r0 < HJ_TILE ? nrows - r0 : HJ_TILE;

        // this lane's columns: c0 + c * 256 + tid.  One past the end re-reads the last row and is marked dead.
        uint64_t col[HJ_CPL][HW];
        uint32_t valid = 0;
#pragma unroll
        for (int c = 0; c < HJ_CPL; ++c) {
            const int j = c0 + c * HJ_THREADS + tid;
            const int jj = j < ncols ? j : ncols - 1;
#pragma unroll
            for (int k = 0; k < HW; ++k) col[c][k] = cside[(int64_t)jj * HW + k];
            uint32_t mw = ~0u;
            if (row_mask) mw = row_mask[jj >> 5];
            valid |= ((uint32_t)(j < ncols) & (mw >> (jj & 31))) << c;
        }

        // the uniform side, RU rows per step; a step past the end re-reads the tile's last row (dropped by index below)
        uint64_t cur[RU][HW];
        if (PREFETCH) {
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int ii = u < rcount ? u : rcount - 1;
#pragma unroll
                for (int k = 0; k < HW; ++k) cur[u][k] = rows[(int64_t)(r0 + ii) * HW + k];
            }
        }
        for (int i = 0; i < rcount; i += RU) {
            uint64_t nxt[RU][HW];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int at = PREFETCH ? i + RU + u : i + u;
                const int ii = at < rcount ? at : rcount - 1;
#pragma unroll
                for (int k = 0; k < HW; ++k) (PREFETCH ? nxt : cur)[u][k] = rows[(int64_t)(r0 + ii) * HW + k];
            }

            // per pair, min over the kinds of (distance - thr): <= 0 iff the pair is within a threshold
            int e[RU][HJ_CPL];
            int m = HJ_OFF;
#pragma unroll
            for (int u = 0; u < RU; ++u)
#pragma unroll
                for (int c = 0; c < HJ_CPL; ++c) {
                    e[u][c] = hash_dist<W>(cur[u], col[c], 0, bias.v[0]);
#pragma unroll
                    for (int h = 1; h < H; ++h) e[u][c] = min(e[u][c], hash_dist<W>(cur[u], col[c], h, bias.v[h]));
                    m = min(m, e[u][c]);
                }

            if (__ballot(m <= 0)) {
                // some pair of this wave's step is within a threshold: keep the pairs that are, under the index rules
                // (sign bits, not comparisons: sixteen lane masks at once do not fit the SGPR file beside the rows)
                uint32_t pred = 0;
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    const int ia = r0 + i + u;
                    uint32_t rowok = i + u < rcount;
                    if (SELF && rowok && row_mask) rowok = (row_mask[ia >> 5] >> (ia & 31)) & 1u;
#pragma unroll
                    for (int c = 0; c < HJ_CPL; ++c) {
                        uint32_t ok = ((uint32_t)(e[u][c] - 1) >> 31) & (valid >> c) & rowok;         // e <= 0, column live
                        if (SELF) ok &= (uint32_t)(ia - (c0 + c * HJ_THREADS + tid)) >> 31;           // i < j
                        pred |= ok << (u * HJ_CPL + c);
                    }
                }
                const WavePrefix wp = wave_prefix(__popc(pred), lane);
                if (wp.total > 0) {
                    unsigned long long wbase = 0;
                    if (lane == 0) wbase = atomicAdd(lists, (unsigned long long)__builtin_amdgcn_readfirstlane(wp.total));
                    wbase = __shfl(wbase, 0, 64);
                    const unsigned long long pos0 = wbase + (unsigned long long)wp.before;
                    uint64_t *keys = (uint64_t *)lists + 32, *vals = keys + ((cap + 31) & ~(int64_t)31);
#pragma unroll
                    for (int u = 0; u < RU; ++u) {
#pragma unroll
                        for (int c = 0; c < HJ_CPL; ++c) {
                            const uint32_t bit = 1u << (u * HJ_CPL + c);
                            const unsigned long long pos = pos0 + (unsigned long long)__popc(pred & (bit - 1u));
                            if ((pred & bit) && pos < (unsigned long long)cap) {
                                uint64_t d = 0;
#pragma unroll
                                for (int h = 0; h < 4; ++h) {
                                    uint64_t dh = 0xFFFFu;
                                    if (h < H && bias.v[h < H ? h : 0] <= 0) dh = (uint64_t)hash_dist_cold<W>(cur[u], col[c], h < H ? h : 0);
                                    d |= dh << (16 * h);
                                }
                                keys[pos] = ((uint64_t)(uint32_t)(r0 + i + u) << 32) | (uint32_t)(c0 + c * HJ_THREADS + tid);
                                vals[pos] = d;
                            }
                        }
                    }
                }
            }
            if (PREFETCH) {
#pragma unroll
                for (int u = 0; u < RU; ++u)
#pragma unroll
                    for (int k = 0; k < HW; ++k) cur[u][k] = nxt[u][k];
            }
        }
    }
}

// sort padding: keys above every real key ((row count) << 32), so they sort last.  The same kernel as row_lists.h's
// fill_u64; it stays here because tests/test_hash_join_isa.py pins this file's kernel set by name.
__global__ __launch_bounds__(256) void hash_fill_kernel(uint64_t *__restrict__ k, int64_t n, uint64_t pad)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) k[i] = pad;
}

__global__ __launch_bounds__(256) void hash_emit_kernel(const unsigned long long *__restrict__ counter, const uint64_t *__restrict__ sk,
                                                        const uint64_t *__restrict__ sv, int64_t cap, int32_t *__restrict__ out_a,
                                                        int32_t *__restrict__ out_b, uint64_t *__restrict__ out_dist,
                                                        int64_t *__restrict__ counts)
{
    const unsigned long long matches = counter[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = (int64_t)matches;
    const int64_t n = matches < (unsigned long long)cap ? (int64_t)matches : cap;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t key = sk[i];
        out_a[i] = (int32_t)(key >> 32);
        out_b[i] = (int32_t)(key & 0xffffffffu);
        if (out_dist) out_dist[i] = sv[i];
    }
}

struct HashPlan {
    size_t off_cnt, off_k, off_v, off_k2, off_v2, off_tmp, tmp_bytes, total;
};

static HashPlan make_hash_plan(int64_t cap)
{
    HashPlan p{};
    const int64_t cc = cap > 0 ? cap : 1;
    WsLayout l;
    p.off_cnt = l.take(256);                                      // the kernel's `lists`: counter, keys, distances
    p.off_k = l.take((size_t)cc * 8);
    p.off_v = l.take((size_t)cc * 8);
    p.off_k2 = l.take((size_t)cc * 8);
    p.off_v2 = l.take((size_t)cc * 8);
    p.tmp_bytes = sort_bytes<uint64_t>(cc);
    p.off_tmp = l.take(p.tmp_bytes > 0 ? p.tmp_bytes : 1);
    p.total = l.off;
    return p;
}

static bool hash_shape_ok(int H, int W) { return H >= 1 && H <= 4 && (W == 1 || W == 4); }

template <bool SELF, class... A>
static int launch_hash_join(int H, int W, unsigned grid, hipStream_t st, A... args)
{
#define MMR_HJ_CASE(h, w)                                                                                          \
    if (H == h && W == w) {                                                                                        \
        hipLaunchKernelGGL((hash_join_kernel<h, w, SELF>), dim3(grid), dim3(HJ_THREADS), 0, st, args...);         \
        MMR_CHECK_LAUNCH();                                                                                        \
        return MMR_OK;                                                                                             \
    }
    MMR_HJ_CASE(1, 1) MMR_HJ_CASE(2, 1) MMR_HJ_CASE(3, 1) MMR_HJ_CASE(4, 1)
    MMR_HJ_CASE(1, 4) MMR_HJ_CASE(2, 4) MMR_HJ_CASE(3, 4) MMR_HJ_CASE(4, 4)
#undef MMR_HJ_CASE
    set_error("hash join: H=%d W=%d unsupported", H, W);
    return MMR_ENOTSUP;
}

// Shared body of mmr_hash_self_join (queries == NULL: the rows pair with themselves) and mmr_hash_cross_join.
static int hash_join_impl(const char *fn, const uint64_t *queries, int64_t M, const uint64_t *refs, int64_t N, int H, int W,
                          const int32_t *thresholds_host, const uint32_t *row_mask, int64_t cap, int32_t *out_a, int32_t *out_b,
                          uint64_t *out_dist, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool self = queries == nullptr;
    MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff, "%s: N=%lld outside [0, 2^31-1)", fn, (long long)N);
    MMR_CHECK_ARG(self || (M >= 0 && M < 0x7fffffff), "%s: M=%lld outside [0, 2^31-1)", fn, (long long)M);
    MMR_CHECK_ARG(H >= 1 && H <= 4, "%s: H=%d must be 1..4 hash kinds", fn, H);
    MMR_CHECK_ARG(W == 1 || W == 4, "%s: W=%d must be 1 or 4 words per hash (zero-pad other sizes)", fn, W);
    MMR_CHECK_ARG(thresholds_host != nullptr, "%s: null pointer (thresholds)", fn);
    HashBias bias;
    bool any = false;
    for (int h = 0; h < 4; ++h) {
        const bool on = h < H && thresholds_host[h] >= 0;
        // a threshold of 64 W or more accepts every pair of that kind; larger values mean the same
        bias.v[h] = on ? -(thresholds_host[h] < 64 * W ? thresholds_host[h] : 64 * W) : HJ_OFF;
        any |= on;
    }
    MMR_CHECK_ARG(any, "%s: every threshold is negative: no hash kind is enabled", fn);
    MMR_CHECK_ARG(cap >= 0, "%s: cap=%lld must be >= 0", fn, (long long)cap);
    MMR_CHECK_ARG(counts != nullptr && workspace != nullptr, "%s: null pointer (counts / workspace)", fn);
    MMR_CHECK_ARG(refs != nullptr || N == 0, "%s: null pointer (hashes)", fn);
    MMR_CHECK_ARG(cap == 0 || (out_a && out_b), "%s: null pointer (outputs)", fn);
    MMR_CHECK_ARG((((uintptr_t)queries | (uintptr_t)refs | (uintptr_t)out_dist | (uintptr_t)counts) & 7) == 0,
                  "%s: hashes / out_dist / counts must be 8-byte aligned", fn);
    MMR_CHECK_ARG((((uintptr_t)out_a | (uintptr_t)out_b | (uintptr_t)row_mask) & 3) == 0,
                  "%s: index outputs and row_mask must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
    const HashPlan p = make_hash_plan(cap);
    if (workspace_bytes < p.total) { set_error("%s: workspace %zu < required %zu", fn, workspace_bytes, p.total); return MMR_ENOSPC; }
    if (p.tmp_bytes == 0) { set_error("%s: sort storage query failed", fn); return MMR_EIO; }

    hipStream_t st = (hipStream_t)stream;
    const int64_t nrows = self ? N : M;
    if ((self && N <= 1) || (!self && (M == 0 || N == 0))) {      // no pair exists: nothing that could read a row is launched
        MMR_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t), st));
        return MMR_OK;
    }
    char *ws = (char *)workspace;
    unsigned long long *counter = (unsigned long long *)(ws + p.off_cnt);
    uint64_t *k1 = (uint64_t *)(ws + p.off_k), *v1 = (uint64_t *)(ws + p.off_v);
    uint64_t *k2 = (uint64_t *)(ws + p.off_k2), *v2 = (uint64_t *)(ws + p.off_v2);
    MMR_CHECK_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
    if (cap > 0) {
        hipLaunchKernelGGL(hash_fill_kernel, dim3(grid_1d(cap)), dim3(256), 0, st, k1, cap, (uint64_t)nrows << 32);
        MMR_CHECK_LAUNCH();
    }
    const int64_t ntr = (nrows + HJ_TILE - 1) / HJ_TILE, ntc = (N + HJ_TILE - 1) / HJ_TILE;
    const int64_t ntiles = self ? ntc * (ntc + 1) / 2 : ntr * ntc;
    const unsigned grid = grid_1d(ntiles, 1, HJ_MAX_GRID);        // ntiles >= 1 here
    {
        ProfScope prof(MMR_PROF_EXACT, st);
        if (self)
            MMR_TRY(launch_hash_join<true>(H, W, grid, st, refs, refs, (int)N, (int)N, (int)ntc, ntiles, bias, row_mask, counter, cap));
        else
            MMR_TRY(launch_hash_join<false>(H, W, grid, st, queries, refs, (int)M, (int)N, (int)ntc, ntiles, bias, row_mask, counter, cap));
    }
    ProfScope prof(MMR_PROF_FINALIZE, st);
    // the appended pairs sit in [0, min(matches, cap)) of k1 / v1, padding behind them: sort on the bits that can differ
    if (cap > 0) MMR_TRY(sort_pairs<uint64_t>(fn, ws + p.off_tmp, p.tmp_bytes, k1, k2, v1, v2, cap, 0, 32 + bitlen64((uint64_t)nrows), st));
    hipLaunchKernelGGL(hash_emit_kernel, dim3(grid_1d(cap)), dim3(256), 0, st,
                       (const unsigned long long *)counter, (const uint64_t *)k2, (const uint64_t *)v2, cap, out_a, out_b, out_dist, counts);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_hash_join_workspace_bytes(int64_t M, int64_t N, int H, int W, int64_t cap)
{
    if (M < 0 || N < 0 || cap < 0 || !hash_shape_ok(H, W)) return 0;
    return make_hash_plan(cap).total;
}

extern "C" int mmr_hash_self_join(const uint64_t *hashes, int64_t N, int H, int W, const int32_t *thresholds_host,
                                  const uint32_t *row_mask, int64_t cap, int32_t *out_i, int32_t *out_j, uint64_t *out_dist,
                                  int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    return hash_join_impl("mmr_hash_self_join", nullptr, 0, hashes, N, H, W, thresholds_host, row_mask, cap, out_i, out_j, out_dist,
                          counts, workspace, workspace_bytes, stream);
}

extern "C" int mmr_hash_cross_join(const uint64_t *queries, int64_t M, const uint64_t *refs, int64_t N, int H, int W,
                                   const int32_t *thresholds_host, const uint32_t *ref_row_mask, int64_t cap, int32_t *out_q,
                                   int32_t *out_ref, uint64_t *out_dist, int64_t *counts, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    if (queries == nullptr && M != 0) { set_error("mmr_hash_cross_join: null pointer (queries)"); return MMR_EINVAL; }
    if (queries == nullptr) {       // M == 0: no pair; still check the rest as a cross join would
        static const uint64_t none = 0;
        queries = &none;
    }
    return hash_join_impl("mmr_hash_cross_join", queries, M, refs, N, H, W, thresholds_host, ref_row_mask, cap, out_q, out_ref,
                          out_dist, counts, workspace, workspace_bytes, stream);
}
