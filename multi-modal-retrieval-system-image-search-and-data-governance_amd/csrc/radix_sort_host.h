// rocPRIM's radix_sort_pairs over uint64 keys behind this library's error codes, for the calls that sort pairs: the range
// search / self-join (range.hip: values fp64), the deep top-k (deep_topk.hip: values uint64), the hash join
// (hash_join.hip: values uint64) and the grouping of rows by label (row_lists.hip: values uint32, for cluster.hip and
// silhouette.hip).  A header of its own so that only those files include rocPRIM's radix sort.
#pragma once
#include "mmr_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace mmr {

static inline int bitlen64(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// temporary storage of a sort of n pairs on all 64 key bits (rocPRIM's own size query; no launch); 0: the query failed
template <class V>
static inline size_t sort_bytes(int64_t n)
{
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const V *)nullptr, (V *)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess)
        return 0;
    return bytes;
}

// (kin, vin) -> (kout, vout), ascending and stable on key bits [begin_bit, end_bit), in `reserved` bytes at tmp: the size
// is queried again for these bits and checked against the reservation
template <class V>
static inline int sort_pairs(const char *fn, void *tmp, size_t reserved, const uint64_t *kin, uint64_t *kout, const V *vin, V *vout,
                             int64_t n, int begin_bit, int end_bit, hipStream_t st)
{
    size_t need = 0;
    MMR_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)n, begin_bit, end_bit, st));
    if (need > reserved) { set_error("%s: sort storage %zu > reserved %zu", fn, need, reserved); return MMR_EIO; }
    need = reserved;
    MMR_CHECK_HIP(rocprim::radix_sort_pairs(tmp, need, kin, kout, vin, vout, (size_t)n, begin_bit, end_bit, st));
    return MMR_OK;
}

}  // namespace mmr
