// Silhouette sums of a labelled gallery for gfx950: sums[i, c] = the sum of d(i, j) over the rows j carrying label c, for
// EVERY row i, in one pairwise scan -- the second line of the reference's K-selection loop (silhouette_score in
// get_cluster_features, reference code/search_image.py:256-259; assign.hip / cluster.hip are the first).  N x N distances
// are computed, none leaves the chip.
//
// Structure ("Silhouette"):
//   silhouette_keys_kernel + sort_label_groups   row ids grouped by label, ascending row id inside a label (row_lists.h)
//   silhouette_plan_kernel    start[k] by binary search, sizes[k]; each cluster's first tile and first chunk in a copy
//                             where every cluster starts on a 32-row tile and a chunk (<= 64 tiles) holds one cluster
//   silhouette_gather_kernel  one wave per sorted row: the row's norm term (|x|^2 exact in fp64, rounded once to fp32;
//                             cosine: 1 / |x|), its copy in the sorted array, its position there; the last row of a
//                             cluster also fills the tile's padding rows with copies of itself
//   silhouette_scan_kernel    range_scan_kernel's ring with a distance epilogue (silhouette_scan_body.h): resident =
//                             256 rows (128 at E = 768) in original order, streamed = one chunk; one fp32 partial per
//                             (chunk, row), at most 1024 + 1 additions each
//   silhouette_final_kernel   sums[i, c] = the partials of c's chunks added in fp64, ascending chunk
//   silhouette_samples_kernel the elementwise rule in fp64
// No floating-point atomics: every addition's order depends on the labels, N and K alone.
#include "mmr_common.h"
#include "row_lists.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "silhouette_scan_body.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

// silhouette_scan_kernel, SilScanArgs and launch_silhouette_scan: silhouette_scan_body.h; the fp16 kernels are compiled in
// silhouette_f16.hip

// row_lists.hip's label_keys_kernel under this file's name: tests/test_silhouette_isa.py pins the kernel set
__global__ __launch_bounds__(256) void silhouette_keys_kernel(const int32_t *__restrict__ labels, int64_t N, int K,
                                                              uint64_t *__restrict__ keys, uint32_t *__restrict__ rows)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        keys[i] = label_key(labels[i], K);
        rows[i] = (uint32_t)i;
    }
}

// One workgroup of 1024 threads, thread k owns cluster k (K <= 1024).  keys: sorted.
__global__ __launch_bounds__(1024) void silhouette_plan_kernel(const uint64_t *__restrict__ keys, int64_t N, int K,
                                                               int64_t *__restrict__ start, int32_t *__restrict__ tstart,
                                                               int32_t *__restrict__ cstart, int64_t *__restrict__ sizes)
{
    __shared__ int32_t pt[1024], pc[1024];
    const int k = threadIdx.x;
    int64_t s[2] = {0, 0};
    if (k < K) {
        for (int j = 0; j < 2; ++j)            // the number of sorted keys below k + j
            s[j] = lower_bound_idx(N, (uint64_t)(k + j), [&](int64_t i) { return keys[i]; });
    }
    const int64_t n = s[1] - s[0];
    const int32_t tiles = (int32_t)((n + RTILE - 1) / RTILE), chunks = (tiles + SIL_TPC - 1) / SIL_TPC;
    pt[k] = tiles;
    pc[k] = chunks;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {             // inclusive prefix sums
        const int32_t vt = k >= off ? pt[k - off] : 0, vc = k >= off ? pc[k - off] : 0;
        __syncthreads();
        pt[k] += vt;
        pc[k] += vc;
        __syncthreads();
    }
    if (k < K) {
        start[k] = s[0];
        tstart[k] = pt[k] - tiles;
        cstart[k] = pc[k] - chunks;
        sizes[k] = n;
        if (k == K - 1) { start[K] = s[1]; tstart[K] = pt[k]; cstart[K] = pc[k]; }
    }
}

// One wave per sorted position s (256 threads = 4 positions a workgroup).
template <typename T>
__global__ __launch_bounds__(256) void silhouette_gather_kernel(const T *__restrict__ gal, int64_t N, int E, int K, int cosine,
                                                                const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rows,
                                                                const int64_t *__restrict__ start, const int32_t *__restrict__ tstart,
                                                                T *__restrict__ sorted, float *__restrict__ nrm,
                                                                float *__restrict__ snrm, int32_t *__restrict__ spos)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= N) return;
    const uint32_t row = rows[s];
    const uint64_t key = keys[s];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(gal + (size_t)row * E);
    const bool live = key < (uint64_t)K;
    int64_t at = 0, copies = 1;
    if (live) {
        const int64_t m = s - start[key], n = start[key + 1] - start[key];
        at = (int64_t)tstart[key] * RTILE + m;
        if (m == n - 1) copies = (int64_t)tstart[key + 1] * RTILE - at;   // the last row fills the padding
    }
    double ss = 0.0;
    for (int e = lane; e < E / 2; e += 64) {
        const uint32_t w = src[e];
        const double x = (double)b16_to_f32<T>((uint16_t)(w & 0xffffu)), y = (double)b16_to_f32<T>((uint16_t)(w >> 16));
        ss += x * x;
        ss += y * y;
        if (live)
            for (int64_t j = 0; j < copies; ++j) reinterpret_cast<uint32_t *>(sorted + (size_t)(at + j) * E)[e] = w;
    }
    ss = wave_sum_f64_butterfly(ss);
    const float v = cosine ? (float)(1.0 / sqrt(ss)) : (float)ss;
    if (lane == 0) {
        nrm[row] = v;
        spos[row] = live ? (int32_t)at : -1;
    }
    if (live)
        for (int64_t j = lane; j < copies; j += 64) snrm[at + j] = v;
}

// 32 rows x 32 clusters a workgroup: the partials are read along i, the sums written along c, through LDS
__global__ __launch_bounds__(1024) void silhouette_final_kernel(const float *__restrict__ partial, const int32_t *__restrict__ cstart,
                                                                int64_t N, int K, double *__restrict__ sums)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    {
        const int64_t i = i0 + tx;
        const int c = c0 + ty;
        double s = 0.0;
        if (i < N && c < K) {
            const int lo = cstart[c], hi = cstart[c + 1];
            for (int ch = lo; ch < hi; ++ch) {
                const double p = (double)partial[(size_t)ch * (size_t)N + (size_t)i];
                s = ch == lo ? p : s + p;
            }
        }
        tile[ty][tx] = s;
    }
    __syncthreads();
    const int64_t i = i0 + ty;
    const int c = c0 + tx;
    if (i < N && c < K) sums[(size_t)i * K + c] = tile[tx][ty];
}

// samples[i] from sums[i, :], labels and sizes: include/mmr.h states the rule.  Divisions, one subtraction, comparisons:
// nothing a compiler could contract, so the result is numpy's bit for bit.
__global__ __launch_bounds__(256) void silhouette_samples_kernel(const double *__restrict__ sums, const int32_t *__restrict__ labels,
                                                                 const int64_t *__restrict__ sizes, int64_t N, int K,
                                                                 double *__restrict__ samples)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int32_t own = labels[i];
        double out = (double)NAN;
        if (own >= 0 && own < K) {
            const int64_t n = sizes[own];
            if (n == 1) {
                out = 0.0;
            } else {
                const double *row = sums + (size_t)i * K;
                const double av = row[own] / (double)(n - 1);
                double bv = (double)INFINITY;
                bool nan = av != av;
                for (int c = 0; c < K; ++c) {
                    const int64_t m = sizes[c];
                    if (c == own || m <= 0) continue;
                    const double v = row[c] / (double)m;
                    nan = nan || v != v;
                    if (v < bv) bv = v;
                }
                const double mx = av > bv ? av : bv;
                out = nan ? (double)NAN : (mx == 0.0 ? 0.0 : (bv - av) / mx);
            }
        }
        samples[i] = out;
    }
}

struct SilPlan {
    int64_t tmax, cmax, nblk, items;
    LabelGroups groups;
    size_t off_start, off_tstart, off_cstart, off_spos, off_nrm, off_snrm, off_sorted, off_partial, total;
};

// tmax: sum_k ceil(n_k / 32) <= N / 32 + (non-empty clusters); cmax: sum_k ceil(tiles_k / 64) likewise.  The grid and the
// partials are sized by them: the labels are not read on the host.
static SilPlan make_sil_plan(int64_t N, int E, int K)
{
    SilPlan p{};
    const int64_t n1 = N > 0 ? N : 1, kn = K < n1 ? K : n1;
    p.tmax = (n1 + RTILE - 1) / RTILE + kn;
    p.cmax = p.tmax / SIL_TPC + kn;
    const int qmax = scan_qmax(E, MMR_BF16);
    p.nblk = (n1 + qmax - 1) / qmax;
    p.items = p.nblk * p.cmax;
    WsLayout l;
    p.groups = reserve_label_groups(l, n1);
    p.off_start = l.take((size_t)(K + 1) * 8);
    p.off_tstart = l.take((size_t)(K + 1) * 4);
    p.off_cstart = l.take((size_t)(K + 1) * 4);
    p.off_spos = l.take((size_t)n1 * 4);
    p.off_nrm = l.take((size_t)n1 * 4);
    p.off_snrm = l.take((size_t)p.tmax * RTILE * 4);
    p.off_sorted = l.take((size_t)p.tmax * RTILE * E * 2);
    p.off_partial = l.take((size_t)p.cmax * (size_t)n1 * 4);
    p.total = l.off;
    return p;
}

}  // namespace mmr

using namespace mmr;

static bool silhouette_sizes_ok(int64_t N, int E, int K, mmr_dtype dtype)
{
    if (!(N >= 0 && N < 0x7fffffff && K >= 1 && K <= MMR_SILHOUETTE_K_MAX && scan_supports_E(E) && (dtype == MMR_BF16 || dtype == MMR_F16)))
        return false;
    return make_sil_plan(N, E, K).items <= 0x7fffffff;      // one launch
}

extern "C" size_t mmr_silhouette_workspace_bytes(int64_t N, int E, int K, mmr_dtype dtype)
{
    if (!silhouette_sizes_ok(N, E, K, dtype)) return 0;
    return make_sil_plan(N, E, K).total;
}

extern "C" int mmr_silhouette_sums(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K, int metric,
                                   double *sums, int64_t *sizes, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_silhouette_sums";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    if (dtype == MMR_F32) {
        set_error("%s: fp32 galleries are not supported (bf16 or fp16 only: the score belongs to the 16-bit gallery the clustering ran on)", fn);
        return MMR_ENOTSUP;
    }
    MMR_TRY(ck.scan_E(E));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(K >= 1 && K <= MMR_SILHOUETTE_K_MAX, "%s: K=%d outside [1, %d]", fn, K, MMR_SILHOUETTE_K_MAX);
    MMR_CHECK_ARG(metric == 0 || metric == 1, "%s: metric=%d (0 = euclidean, 1 = cosine)", fn, metric);
    MMR_CHECK_ARG(sizes != nullptr && workspace != nullptr, "%s: null pointer (sizes / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr && sums != nullptr) || N == 0, "%s: null pointer (gallery / labels / sums)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)gallery, "gallery"));
    MMR_CHECK_ARG((((uintptr_t)sums | (uintptr_t)sizes) & 7) == 0, "%s: sums / sizes must be 8-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)labels & 3) == 0, "%s: labels must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    const SilPlan p = make_sil_plan(N, E, K);
    if (p.items > 0x7fffffff) {
        set_error("%s: N=%lld with K=%d needs more work items than one launch holds (shard the gallery)", fn, (long long)N, K);
        return MMR_ENOTSUP;
    }
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {       // no rows: no sums; only the sizes are written
        MMR_CHECK_HIP(hipMemsetAsync(sizes, 0, (size_t)K * sizeof(int64_t), st));
        return MMR_OK;
    }
    char *ws = (char *)workspace;
    const uint64_t *keys2 = p.groups.sorted_keys(ws);
    const uint32_t *rows2 = p.groups.sorted_rows(ws);
    SilScanArgs a{};
    a.gal = (const bf16_t *)gallery;
    a.sorted = (const bf16_t *)(ws + p.off_sorted);
    a.N = N;
    a.spad = p.tmax * RTILE;
    a.K = K;
    a.nblk = (int)p.nblk;
    a.start = (const int64_t *)(ws + p.off_start);
    a.tstart = (const int32_t *)(ws + p.off_tstart);
    a.cstart = (const int32_t *)(ws + p.off_cstart);
    a.nrm = (const float *)(ws + p.off_nrm);
    a.snrm = (const float *)(ws + p.off_snrm);
    a.spos = (const int32_t *)(ws + p.off_spos);
    a.partial = (float *)(ws + p.off_partial);

    {
        ProfScope prof(MMR_PROF_FINALIZE, st);
        hipLaunchKernelGGL(silhouette_keys_kernel, dim3(grid_1d(N)), dim3(256), 0, st, labels, N, K, p.groups.keys(ws), p.groups.rows(ws));
        MMR_CHECK_LAUNCH();
        MMR_TRY(sort_label_groups(fn, ws, p.groups, N, K, st));
        hipLaunchKernelGGL(silhouette_plan_kernel, dim3(1), dim3(1024), 0, st, keys2, N, K, (int64_t *)a.start,
                           (int32_t *)a.tstart, (int32_t *)a.cstart, sizes);
        MMR_CHECK_LAUNCH();
        const dim3 ggrid((unsigned)((N + 3) / 4));
        if (dtype == MMR_F16)
            hipLaunchKernelGGL(silhouette_gather_kernel<f16_t>, ggrid, dim3(256), 0, st, (const f16_t *)gallery, N, E, K, metric,
                               keys2, rows2, a.start, a.tstart, (f16_t *)(ws + p.off_sorted),
                               (float *)a.nrm, (float *)a.snrm, (int32_t *)a.spos);
        else
            hipLaunchKernelGGL(silhouette_gather_kernel<bf16_t>, ggrid, dim3(256), 0, st, (const bf16_t *)gallery, N, E, K, metric,
                               keys2, rows2, a.start, a.tstart, (bf16_t *)(ws + p.off_sorted),
                               (float *)a.nrm, (float *)a.snrm, (int32_t *)a.spos);
        MMR_CHECK_LAUNCH();
    }
    MMR_TRY(dtype == MMR_F16 ? launch_silhouette_scan<f16_t>(E, metric, a, (unsigned)p.items, st)
                             : launch_silhouette_scan<bf16_t>(E, metric, a, (unsigned)p.items, st));
    ProfScope prof(MMR_PROF_FINALIZE, st);
    const dim3 fgrid((unsigned)((N + 31) / 32), (unsigned)((K + 31) / 32));
    hipLaunchKernelGGL(silhouette_final_kernel, fgrid, dim3(1024), 0, st, (const float *)a.partial, a.cstart, N, K, sums);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

extern "C" int mmr_silhouette_samples(const double *sums, const int32_t *labels, const int64_t *sizes, int64_t N, int K,
                                      double *samples, void *stream)
{
    const char *fn = "mmr_silhouette_samples";
    const EntryCheck ck{fn};
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(K >= 1 && K <= MMR_SILHOUETTE_K_MAX, "%s: K=%d outside [1, %d]", fn, K, MMR_SILHOUETTE_K_MAX);
    if (N == 0) return MMR_OK;
    MMR_CHECK_ARG(sums != nullptr && labels != nullptr && sizes != nullptr && samples != nullptr, "%s: null pointer", fn);
    MMR_CHECK_ARG((((uintptr_t)sums | (uintptr_t)sizes | (uintptr_t)samples) & 7) == 0, "%s: sums / sizes / samples must be 8-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)labels & 3) == 0, "%s: labels must be 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_FINALIZE, st);
    hipLaunchKernelGGL(silhouette_samples_kernel, dim3(grid_1d(N)), dim3(256), 0, st, sums, labels, sizes, N, K, samples);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
