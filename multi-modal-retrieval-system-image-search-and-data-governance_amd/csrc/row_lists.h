// Lists of rows on the device, the parts more than one call builds the same way (kernels: row_lists.hip):
//   fill_u64          the padding keys behind a capped pair list before its sort: mmr_cosine_range* / mmr_gallery_self_join*
//                     (range.hip), mmr_hash_join* (hash_join.hip), mmr_cosine_topk_deep (deep_topk.hip)
//   lower_bound_idx   the binary search behind every start[k]: label_bounds below, silhouette_plan_kernel (silhouette.hip),
//                     rank_bounds_kernel (cluster_rank.hip)
//   LabelGroups       rows grouped by label -- keys from the labels, a stable radix sort, the groups' starts:
//                     mmr_cluster_sums (cluster.hip) and mmr_silhouette_sums (silhouette.hip, which writes the keys with a
//                     kernel of its own name and finds the starts in its plan kernel)
#pragma once
#include "mmr_common.h"

namespace mmr {

// k[0, n) = pad; the hash join (hash_join.hip) keeps a fill kernel of its own name
int fill_u64(uint64_t *k, int64_t n, uint64_t pad, hipStream_t st);

// The first index in [0, n) whose key is not below k (n: every key is below it); key(i) reads an ascending sequence.
template <class Key>
__device__ __forceinline__ int64_t lower_bound_idx(int64_t n, uint64_t k, Key key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key(mid) < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The grouping key of a row: its label, K for a label outside [0, K).  The value sorted with it is the row id.
__device__ __forceinline__ uint64_t label_key(int32_t l, int K) { return (l >= 0 && l < K) ? (uint64_t)l : (uint64_t)K; }

// The workspace slots of one grouping of N rows (n1 = max(N, 1)): the keys and row ids before and after the sort, and the
// sort's storage
struct LabelGroups {
    size_t off_keys, off_keys2, off_rows, off_rows2, off_sort, sort_bytes;
    uint64_t *keys(char *ws) const { return (uint64_t *)(ws + off_keys); }
    uint32_t *rows(char *ws) const { return (uint32_t *)(ws + off_rows); }
    const uint64_t *sorted_keys(const char *ws) const { return (const uint64_t *)(ws + off_keys2); }
    const uint32_t *sorted_rows(const char *ws) const { return (const uint32_t *)(ws + off_rows2); }
};
LabelGroups reserve_label_groups(WsLayout &l, int64_t n1);

// (keys, rows) = (label_key, row id) of rows [0, N), already written: one stable sort on bitlen64(K) bits leaves the
// keys ascending in sorted_keys and, inside a label, the row ids ascending in sorted_rows
int sort_label_groups(const char *fn, char *ws, const LabelGroups &g, int64_t N, int K, hipStream_t st);
// the keys and row ids from the labels, then sort_label_groups
int group_rows_by_label(const char *fn, char *ws, const LabelGroups &g, const int32_t *labels, int64_t N, int K, hipStream_t st);

// start[k], k in [0, K]: the number of sorted keys below k
int label_bounds(const uint64_t *sorted_keys, int64_t N, int K, int64_t *start, hipStream_t st);

}  // namespace mmr
