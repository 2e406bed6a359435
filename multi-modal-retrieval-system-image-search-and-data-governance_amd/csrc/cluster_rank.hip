// Every row's exact distance to its own cluster's centre, each cluster's rows in order of that distance, and numpy's
// percentile of those distances per cluster, for gfx950: the reference's outlier_filter (code/search_image.py:295-318)
// and the "shots nearest their centre" half of get_cluster_features (185-232) for a gallery instead of ten rows.  The
// definitions are the comments above mmr_cluster_rank and mmr_cluster_percentile_trim in include/mmr.h; DESIGN.md
// section 3, "Distances to the own centre", has the measurements.
//
// mmr_cluster_rank:
//   rank_cnorm_kernel    n_c = dot64(c, c) of every centre (euclidean only)
//   rank_dist_kernel     ONE pass over the gallery in row order: 16 lanes per row, four rows per wave pass (exact_dot.h's
//                        quarter-wave order); a group of 16 lanes walks 16 consecutive rows and keeps the centre in
//                        registers while the label repeats.  Writes dist[row] and the row's sort record
//                        (label or K, sortable image of the distance, row id).
//   merge sort           of the 16-byte records by (label, image, row id): one sort gives every cluster's rows in order
//                        of (distance, row id) and the rows that are not live behind them in row order.  One sort of wide
//                        records, not a grouping sort, a sort by image and a sort by label: rocPRIM sorts a million
//                        64-bit keys by a block sort and ten merge passes whatever the number of key bits asked for
//                        (0.18 ms each at 1M rows), so a sort's cost is its count of rows, not of bits.
//   rank_order_kernel    order[p] = the row of sorted record p
//   rank_bounds_kernel   start[k] by binary search on the records' labels
// mmr_cluster_percentile_trim: one thread per cluster interpolates the threshold and counts the kept rows by binary search
// in the cluster's sorted segment; one thread per row writes its trimmed label.  No atomics at all.
// Vector stores and plain C++ only.
#include "mmr_common.h"
#include "exact_dot.h"
#include "row_lists.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>

namespace mmr {

constexpr int CR_ROWS = 256;             // rows per workgroup of the pass: 16 groups of 16 lanes, 16 rows each
constexpr int CR_K_MAX = 65535;

struct RankRecord {
    uint64_t image;                      // rank_image of the distance
    uint32_t label;                      // the row's label, K for a row that is not live
    uint32_t row;
};
static_assert(sizeof(RankRecord) == 16, "one 16-byte store per row");

// a total order: no two records compare equal, so the sort's stability is not relied on
struct RankLess {
    __host__ __device__ bool operator()(const RankRecord &a, const RankRecord &b) const
    {
        if (a.label != b.label) return a.label < b.label;
        if (a.image != b.image) return a.image < b.image;
        return a.row < b.row;
    }
};

// temporary storage of the sort of n records (rocPRIM's own size query; no launch); 0: the query failed
static inline size_t rank_sort_bytes(int64_t n)
{
    size_t bytes = 0;
    if (rocprim::merge_sort(nullptr, bytes, (RankRecord *)nullptr, (RankRecord *)nullptr, (size_t)n, RankLess{}, (hipStream_t)0) != hipSuccess)
        return 0;
    return bytes;
}

__device__ __forceinline__ double rank_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ascending in (distance, NaN last): the order-preserving image of the distance, all ones for NaN (above +inf's image)
__device__ __forceinline__ uint64_t rank_image(double d) { return d == d ? ord_f64(d) : ~0ull; }

// cnorm[k] = dot64(c_k, c_k): one group of 16 lanes per centre
template <int PER>
__global__ __launch_bounds__(256) void rank_cnorm_kernel(const float *__restrict__ centers, int K, double *__restrict__ cnorm)
{
    constexpr int E = PER * 64;
    const int m = threadIdx.x & 15;
    const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int lk = k < K ? k : K - 1;
    QuadRow<float, PER> c;
    c.load_f32(centers + (size_t)lk * E, m);
    const double n = quad_norm<float, PER>(c);
    if (k < K && m == 0) cnorm[k] = n;
}

// Workgroup b owns the rows [256 b, 256 b + 256); group g of 16 lanes owns [256 b + 16 g, 256 b + 16 g + 16).
template <typename T, int PER>
__global__ __launch_bounds__(CR_ROWS) void rank_dist_kernel(const T *__restrict__ gal, int64_t N, int K,
                                                            const int32_t *__restrict__ labels, const float *__restrict__ centers,
                                                            const double *__restrict__ cnorm, int metric,
                                                            double *__restrict__ dist, RankRecord *__restrict__ records)
{
    constexpr int E = PER * 64;
    const int m = threadIdx.x & 15;
    const int64_t base = (int64_t)blockIdx.x * CR_ROWS + (threadIdx.x >> 4) * 16;
    QuadQuery<T, PER> cq;
    double nc = 0.0;
    int cur = -1;
    for (int p = 0; p < 16; ++p) {
        const int64_t row = base + p;
        const bool valid = row < N;
        const int64_t lrow = valid ? row : N - 1;
        const int32_t lab = labels[lrow];
        const bool live = lab >= 0 && lab < K;
        const int cl = live ? lab : 0;                // a row that is not live is dotted with centre 0 and gets NaN below
        if (cl != cur) {                              // the same for all 16 lanes of the group
            cq.load_f32(centers + (size_t)cl * E, m);
            if (metric == 0) nc = cnorm[cl];
            cur = cl;
        }
        QuadRow<T, PER> gr;
        gr.load(gal + (size_t)lrow * E, m);
        const double s = quad_dot<T, PER>(cq, gr);
        double d;
        if (metric == 0) {
            const double nr = quad_norm<T, PER>(gr);
            d = (nr + nc) - 2.0 * s;                  // 2 s is exact: a contraction into an fma changes nothing
            d = d < 0.0 ? 0.0 : d;
        } else {
            d = 1.0 - s;
        }
        if (d == 0.0) d = 0.0;                        // -0.0 counts as +0.0
        if (!live || !(d == d)) d = rank_nan();
        if (valid && m == 0) {
            dist[row] = d;
            records[row] = RankRecord{rank_image(d), live ? (uint32_t)lab : (uint32_t)K, (uint32_t)row};
        }
    }
}

__global__ __launch_bounds__(256) void rank_order_kernel(const RankRecord *__restrict__ sorted, int64_t N, int32_t *__restrict__ order)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) order[i] = (int32_t)sorted[i].row;
}

// start[k], k in [0, K]: the number of sorted records whose label is below k
__global__ __launch_bounds__(256) void rank_bounds_kernel(const RankRecord *__restrict__ sorted, int64_t N, int K,
                                                          int64_t *__restrict__ start)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    start[k] = lower_bound_idx(N, (uint64_t)k, [&](int64_t i) { return (uint64_t)sorted[i].label; });
}

// One thread per cluster: numpy's linear-interpolation percentile of the sorted segment, every step its own IEEE
// operation, and the number of rows at or below it.  The function is compiled without contraction: hipcc's default fuses
// a + diff * t into an fma, which changes the last bit, and HIP's __dmul_rn / __dadd_rn are plain operators that fuse
// just the same once inlined.  qf = q / 100.0, divided on the host.  Every index is clamped: the buffers are the caller's.
__global__ __launch_bounds__(256) void trim_threshold_kernel(const double *__restrict__ dist, const int32_t *__restrict__ order,
                                                             const int64_t *__restrict__ start, int64_t N, int K, double qf,
                                                             double *__restrict__ thresholds, int64_t *__restrict__ kept)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    int64_t s0 = start[k], s1 = start[k + 1];
    s0 = s0 < 0 ? 0 : (s0 > N ? N : s0);
    s1 = s1 < s0 ? s0 : (s1 > N ? N : s1);
    const int64_t n = s1 - s0;
    auto at = [&](int64_t i) -> double {
        const int32_t r = order[s0 + i];
        return dist[r < 0 ? 0 : ((int64_t)r >= N ? N - 1 : (int64_t)r)];
    };
    double thr = rank_nan();
    int64_t cnt = 0;
    if (n > 0) {
        const double last = at(n - 1);
        if (last == last) {                           // NaN sorts last: a cluster holding one has a NaN threshold
            const double v = qf * (double)(n - 1);
            const double fl = floor(v);
            int64_t lo = (int64_t)fl;
            lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
            const int64_t hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
            const double t = v - fl;
            const double a = at(lo), b = at(hi);
            const double diff = b - a;
            thr = t < 0.5 ? a + diff * t : b - diff * (1.0 - t);
            if (!(thr == thr)) thr = rank_nan();
            int64_t l = 0, h = n;                     // the first sorted position whose distance is not <= thr
            while (l < h) {
                const int64_t mid = (l + h) >> 1;
                if (at(mid) <= thr) l = mid + 1; else h = mid;
            }
            cnt = l;
        }
    }
    thresholds[k] = thr;
    kept[k] = cnt;
}

__global__ __launch_bounds__(256) void trim_labels_kernel(const double *__restrict__ dist, const int32_t *__restrict__ labels,
                                                          const double *__restrict__ thresholds, int64_t N, int K,
                                                          int32_t *__restrict__ trimmed)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int32_t l = labels[i];
        const bool live = l >= 0 && l < K;
        trimmed[i] = (live && dist[i] <= thresholds[live ? l : 0]) ? l : -1;
    }
}

struct RankPlan {
    size_t off_rec, off_rec2, off_cnorm, off_sort, sort_bytes, total;
};

static RankPlan make_rank_plan(int64_t N, int K)
{
    RankPlan p{};
    const int64_t n1 = N > 0 ? N : 1;
    WsLayout l;
    p.off_rec = l.take((size_t)n1 * sizeof(RankRecord));
    p.off_rec2 = l.take((size_t)n1 * sizeof(RankRecord));
    p.off_cnorm = l.take((size_t)K * 8);
    p.off_sort = l.take(rank_sort_bytes(n1));
    p.sort_bytes = l.off - p.off_sort;
    p.total = l.off;
    return p;
}

template <typename T, int PER>
static int rank_run(const char *fn, const T *gal, int64_t N, const int32_t *labels, int K, const float *centers, int metric,
                    double *dist, int32_t *order, int64_t *start, char *ws, const RankPlan &p, hipStream_t st)
{
    RankRecord *rec = (RankRecord *)(ws + p.off_rec), *rec2 = (RankRecord *)(ws + p.off_rec2);
    double *cnorm = (double *)(ws + p.off_cnorm);

    if (metric == 0) {
        hipLaunchKernelGGL((rank_cnorm_kernel<PER>), dim3((unsigned)((K + 15) / 16)), dim3(256), 0, st, centers, K, cnorm);
        MMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((rank_dist_kernel<T, PER>), dim3((unsigned)((N + CR_ROWS - 1) / CR_ROWS)), dim3(CR_ROWS), 0, st, gal, N, K,
                       labels, centers, (const double *)cnorm, metric, dist, rec);
    MMR_CHECK_LAUNCH();
    size_t need = 0;
    MMR_CHECK_HIP(rocprim::merge_sort(nullptr, need, rec, rec2, (size_t)N, RankLess{}, st));
    if (need > p.sort_bytes) { set_error("%s: sort storage %zu > reserved %zu", fn, need, p.sort_bytes); return MMR_EIO; }
    need = p.sort_bytes;
    MMR_CHECK_HIP(rocprim::merge_sort(ws + p.off_sort, need, rec, rec2, (size_t)N, RankLess{}, st));
    hipLaunchKernelGGL(rank_order_kernel, dim3(grid_1d(N)), dim3(256), 0, st, (const RankRecord *)rec2, N, order);
    MMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(rank_bounds_kernel, dim3((unsigned)(K / 256 + 1)), dim3(256), 0, st, (const RankRecord *)rec2, N, K, start);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

static bool rank_sizes_ok(int64_t N, int E, int K)
{
    return N >= 0 && N < 0x7fffffff && scan_supports_E(E) && K >= 1 && K <= CR_K_MAX;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_cluster_rank_workspace_bytes(int64_t N, int E, int K)
{
    if (!rank_sizes_ok(N, E, K)) return 0;
    return make_rank_plan(N, K).total;
}

extern "C" int mmr_cluster_rank(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K,
                                const float *centers, int metric, double *dist, int32_t *order, int64_t *start,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_cluster_rank";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.rows_int32(N));
    MMR_TRY(ck.scan_E(E));
    MMR_CHECK_ARG(K >= 1 && K <= CR_K_MAX, "%s: K=%d outside [1, 65535]", fn, K);
    MMR_CHECK_ARG(metric == 0 || metric == 1, "%s: metric=%d (0 euclidean, 1 cosine)", fn, metric);
    MMR_CHECK_ARG(start != nullptr && workspace != nullptr, "%s: null pointer (start / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr && centers != nullptr) || N == 0, "%s: null pointer (gallery / labels / centers)", fn);
    MMR_CHECK_ARG((dist != nullptr && order != nullptr) || N == 0, "%s: null pointer (dist / order)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)gallery | (uintptr_t)centers, "gallery / centers"));
    MMR_CHECK_ARG((((uintptr_t)dist | (uintptr_t)start) & 7) == 0, "%s: dist / start must be 8-byte aligned", fn);
    MMR_CHECK_ARG((((uintptr_t)labels | (uintptr_t)order) & 3) == 0, "%s: labels / order must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    const RankPlan p = make_rank_plan(N, K);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        MMR_CHECK_HIP(hipMemsetAsync(start, 0, (size_t)(K + 1) * sizeof(int64_t), st));
        return MMR_OK;
    }
    ProfScope prof(MMR_PROF_ROWWISE, st);
    return dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return dispatch_per(E, [&](auto per) -> int {
            constexpr int PER = decltype(per)::value;
            if constexpr (PER == 16) {
                return MMR_ENOTSUP;   // E = 1024: refused by scan_E above
            } else {
                return rank_run<T, PER>(fn, (const T *)gallery, N, labels, K, centers, metric, dist, order, start, (char *)workspace, p, st);
            }
        });
    });
}

extern "C" int mmr_cluster_percentile_trim(const double *dist, const int32_t *order, const int64_t *start, const int32_t *labels,
                                           int64_t N, int K, double q, double *thresholds, int32_t *trimmed_labels,
                                           int64_t *kept, void *stream)
{
    const char *fn = "mmr_cluster_percentile_trim";
    const EntryCheck ck{fn};
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(K >= 1 && K <= CR_K_MAX, "%s: K=%d outside [1, 65535]", fn, K);
    MMR_CHECK_ARG(q >= 0.0 && q <= 100.0, "%s: q=%g outside [0, 100]", fn, q);
    MMR_CHECK_ARG(start != nullptr && thresholds != nullptr && kept != nullptr, "%s: null pointer (start / thresholds / kept)", fn);
    MMR_CHECK_ARG((dist != nullptr && order != nullptr && labels != nullptr && trimmed_labels != nullptr) || N == 0,
                  "%s: null pointer (dist / order / labels / trimmed_labels)", fn);
    MMR_CHECK_ARG((((uintptr_t)dist | (uintptr_t)start | (uintptr_t)thresholds | (uintptr_t)kept) & 7) == 0,
                  "%s: dist / start / thresholds / kept must be 8-byte aligned", fn);
    MMR_CHECK_ARG((((uintptr_t)order | (uintptr_t)labels | (uintptr_t)trimmed_labels) & 3) == 0,
                  "%s: order / labels / trimmed_labels must be 4-byte aligned", fn);

    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    hipLaunchKernelGGL(trim_threshold_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, dist, order, start, N, K, q / 100.0,
                       thresholds, kept);
    MMR_CHECK_LAUNCH();
    if (N > 0) {
        hipLaunchKernelGGL(trim_labels_kernel, dim3(grid_1d(N)), dim3(256), 0, st, dist, labels, (const double *)thresholds, N, K,
                           trimmed_labels);
        MMR_CHECK_LAUNCH();
    }
    return MMR_OK;
}
