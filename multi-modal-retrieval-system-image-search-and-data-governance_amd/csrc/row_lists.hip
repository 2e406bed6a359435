// The kernels and launches behind row_lists.h: the fill of a pair list's padding keys and the grouping of rows by label.
// Vector stores and plain C++ only.
#include "row_lists.h"
#include "radix_sort_host.h"

#include <hip/hip_runtime.h>

namespace mmr {

__global__ __launch_bounds__(256) void fill_u64_kernel(uint64_t *__restrict__ k, int64_t n, uint64_t pad)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) k[i] = pad;
}

__global__ __launch_bounds__(256) void label_keys_kernel(const int32_t *__restrict__ labels, int64_t N, int K,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ rows)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        keys[i] = label_key(labels[i], K);
        rows[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void label_bounds_kernel(const uint64_t *__restrict__ keys, int64_t N, int K,
                                                           int64_t *__restrict__ start)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    start[k] = lower_bound_idx(N, (uint64_t)k, [&](int64_t i) { return keys[i]; });
}

int fill_u64(uint64_t *k, int64_t n, uint64_t pad, hipStream_t st)
{
    hipLaunchKernelGGL(fill_u64_kernel, dim3(grid_1d(n)), dim3(256), 0, st, k, n, pad);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

LabelGroups reserve_label_groups(WsLayout &l, int64_t n1)
{
    LabelGroups g{};
    g.off_keys = l.take((size_t)n1 * 8);
    g.off_keys2 = l.take((size_t)n1 * 8);
    g.off_rows = l.take((size_t)n1 * 4);
    g.off_rows2 = l.take((size_t)n1 * 4);
    g.off_sort = l.take(sort_bytes<uint32_t>(n1));
    g.sort_bytes = l.off - g.off_sort;
    return g;
}

int sort_label_groups(const char *fn, char *ws, const LabelGroups &g, int64_t N, int K, hipStream_t st)
{
    return sort_pairs<uint32_t>(fn, ws + g.off_sort, g.sort_bytes, g.keys(ws), (uint64_t *)(ws + g.off_keys2), g.rows(ws),
                                (uint32_t *)(ws + g.off_rows2), N, 0, bitlen64((uint64_t)K), st);
}

int group_rows_by_label(const char *fn, char *ws, const LabelGroups &g, const int32_t *labels, int64_t N, int K, hipStream_t st)
{
    hipLaunchKernelGGL(label_keys_kernel, dim3(grid_1d(N)), dim3(256), 0, st, labels, N, K, g.keys(ws), g.rows(ws));
    MMR_CHECK_LAUNCH();
    return sort_label_groups(fn, ws, g, N, K, st);
}

int label_bounds(const uint64_t *sorted_keys, int64_t N, int K, int64_t *start, hipStream_t st)
{
    hipLaunchKernelGGL(label_bounds_kernel, dim3((unsigned)(K / 256 + 1)), dim3(256), 0, st, sorted_keys, N, K, start);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr
