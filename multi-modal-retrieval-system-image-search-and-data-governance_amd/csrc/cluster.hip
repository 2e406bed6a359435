// Per-cluster fp64 sums and sizes of labelled gallery rows for gfx950: the second half of a Lloyd iteration
// (KMeans in get_cluster_features, reference code/search_image.py:185-292; assign.hip is the first half).
//
// Bit-for-bit reproducible: no floating-point atomics, and the order of every addition depends on the labels, N and K
// alone ("Nearest-centroid assignment"):
//   group_rows_by_label     key = the row's label, K for a label outside [0, K); value = the row id; a stable radix sort
//                           groups the rows by label, ascending row id inside a label (row_lists.h)
//   label_bounds            start[k] = first sorted position of label k, by binary search
//   cluster_partial_kernel  a cluster's rows in sorted order are cut into chunks of 256; slot y of Y sums the chunks
//                           y, y + Y, ...: each chunk row by row from 0.0, the chunks' sums one after another
//   cluster_final_kernel    sums[k, e] = the slots' partials added in ascending y
// One thread owns one column of one slot, so every sum is a plain sequential fp64 loop.
#include "mmr_common.h"
#include "row_lists.h"
#include "scan_host.h"

#include <hip/hip_runtime.h>

namespace mmr {

constexpr int CL_CHUNK = 256;        // rows per chunk
constexpr int CL_YMAX = 64;          // slots per cluster, at most

// slots per cluster: about one per chunk of an average cluster; a function of N and K alone
static inline int cluster_slots(int64_t N, int K)
{
    const int64_t y = (N / CL_CHUNK + K - 1) / K;
    return (int)(y < 1 ? 1 : (y > CL_YMAX ? CL_YMAX : y));
}

template <typename T>
__device__ __forceinline__ double elem_f64(const T *p)
{
    if constexpr (__is_same(T, float)) return (double)*p;
    else return (double)b16_to_f32<T>(__builtin_bit_cast(uint16_t, *p));
}

// grid (K, Y, ceil(E / 256)): thread t owns column z * 256 + t of slot y of cluster k
template <typename T>
__global__ __launch_bounds__(256) void cluster_partial_kernel(const T *__restrict__ gal, int E, const uint32_t *__restrict__ rows,
                                                              const int64_t *__restrict__ start, int Y,
                                                              double *__restrict__ partial)
{
    __shared__ uint32_t rid[CL_CHUNK];
    const int k = blockIdx.x, y = blockIdx.y;
    const int e = blockIdx.z * 256 + threadIdx.x;
    const bool col = e < E;
    const int64_t s0 = start[k], s1 = start[k + 1];
    const int64_t nch = (s1 - s0 + CL_CHUNK - 1) / CL_CHUNK;
    double acc = 0.0;
    for (int64_t j = y; j < nch; j += Y) {
        const int64_t base = s0 + j * CL_CHUNK;
        const int cnt = (int)(s1 - base < CL_CHUNK ? s1 - base : CL_CHUNK);
        __syncthreads();
        if ((int)threadIdx.x < cnt) rid[threadIdx.x] = rows[base + threadIdx.x];
        __syncthreads();
        double c = 0.0;
        if (col) {
#pragma unroll 8
            for (int i = 0; i < cnt; ++i) c += elem_f64<T>(gal + (size_t)rid[i] * E + e);
        }
        acc = j == y ? c : acc + c;
    }
    if (col && y < nch) partial[((size_t)k * Y + y) * E + e] = acc;
}

__global__ __launch_bounds__(256) void cluster_final_kernel(const double *__restrict__ partial, const int64_t *__restrict__ start,
                                                            int K, int E, int Y, double *__restrict__ sums,
                                                            int64_t *__restrict__ sizes)
{
    const int64_t total = (int64_t)K * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i / E), e = (int)(i % E);
        const int64_t n = start[k + 1] - start[k];
        const int64_t nch = (n + CL_CHUNK - 1) / CL_CHUNK;
        const int ny = (int)(nch < Y ? nch : Y);
        double s = 0.0;
        for (int y = 0; y < ny; ++y) {
            const double p = partial[((size_t)k * Y + y) * E + e];
            s = y == 0 ? p : s + p;
        }
        sums[i] = s;
        if (e == 0) sizes[k] = n;
    }
}

struct ClusterPlan {
    int Y;
    LabelGroups groups;
    size_t off_start, off_partial, total;
};

static ClusterPlan make_cluster_plan(int64_t N, int E, int K)
{
    ClusterPlan p{};
    p.Y = cluster_slots(N, K);
    const int64_t n1 = N > 0 ? N : 1;
    WsLayout l;
    p.groups = reserve_label_groups(l, n1);
    p.off_start = l.take((size_t)(K + 1) * 8);
    p.off_partial = l.take((size_t)K * p.Y * E * 8);
    p.total = l.off;
    return p;
}

constexpr int CLUSTER_K_MAX = 65535;     // grid.x of the partial sums
constexpr int CLUSTER_E_MAX = 65536;

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_cluster_sums_workspace_bytes(int64_t N, int E, int K)
{
    if (N < 0 || N >= 0x7fffffff || K < 1 || K > CLUSTER_K_MAX || E < 1 || E > CLUSTER_E_MAX) return 0;
    return make_cluster_plan(N, E, K).total;
}

extern "C" int mmr_cluster_sums(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K,
                                double *sums, int64_t *sizes, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_cluster_sums";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    MMR_TRY(ck.rows_int32(N));
    MMR_CHECK_ARG(E >= 1 && E <= CLUSTER_E_MAX, "%s: E=%d outside [1, 65536]", fn, E);
    MMR_CHECK_ARG(K >= 1 && K <= CLUSTER_K_MAX, "%s: K=%d outside [1, 65535]", fn, K);
    MMR_CHECK_ARG(sums != nullptr && sizes != nullptr && workspace != nullptr, "%s: null pointer (sums / sizes / workspace)", fn);
    MMR_CHECK_ARG((gallery != nullptr && labels != nullptr) || N == 0, "%s: null pointer (gallery / labels)", fn);
    MMR_CHECK_ARG((((uintptr_t)sums | (uintptr_t)sizes) & 7) == 0, "%s: sums / sizes must be 8-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)gallery & (dtype == MMR_F32 ? 3 : 1)) == 0, "%s: gallery / labels must be aligned to their elements", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    const ClusterPlan p = make_cluster_plan(N, E, K);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        MMR_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)K * E * sizeof(double), st));
        MMR_CHECK_HIP(hipMemsetAsync(sizes, 0, (size_t)K * sizeof(int64_t), st));
        return MMR_OK;
    }
    char *ws = (char *)workspace;
    int64_t *start = (int64_t *)(ws + p.off_start);
    double *partial = (double *)(ws + p.off_partial);

    ProfScope prof(MMR_PROF_ROWWISE, st);
    MMR_TRY(group_rows_by_label(fn, ws, p.groups, labels, N, K, st));
    MMR_TRY(label_bounds(p.groups.sorted_keys(ws), N, K, start, st));
    const dim3 pgrid((unsigned)K, (unsigned)p.Y, (unsigned)((E + 255) / 256));
    MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(cluster_partial_kernel<T>, pgrid, dim3(256), 0, st, (const T *)gallery, E, p.groups.sorted_rows(ws),
                           (const int64_t *)start, p.Y, partial);
        return MMR_OK;
    }));
    MMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cluster_final_kernel, dim3(grid_1d((int64_t)K * E)), dim3(256), 0, st, (const double *)partial,
                       (const int64_t *)start, K, E, p.Y, sums, sizes);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
