// Threshold search and self-join over fp16 galleries for gfx950: range_scan_kernel (range.hip) with fp16 operands.  Same
// body (range_scan_body.inc), same candidate list; range.hip's recheck reads the fp16 rows.  A translation unit of its own:
// the kernel set of range.hip is counted by the ISA tests.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "range_scan_body.h"
#include "scan_f16.h"

namespace mmr {

template <int E, bool TRI, bool MASKED>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void range_scan_f16_kernel(RangeScanArgs a)
{
    using ET = f16_t;
#include "range_scan_body.inc"
}

template <bool TRI>
static int launch_range_scan_f16_t(int E, const RangeScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        if (a.row_mask) return launch_scan_kernel<&range_scan_f16_kernel<decltype(e)::value, TRI, true>>(grid, C::THREADS, C::LDS, st, a);
        return launch_scan_kernel<&range_scan_f16_kernel<decltype(e)::value, TRI, false>>(grid, C::THREADS, C::LDS, st, a);
    });
}

int launch_range_scan_f16(int E, bool tri, const RangeScanArgs &a, unsigned grid, hipStream_t st)
{
    return tri ? launch_range_scan_f16_t<true>(E, a, grid, st) : launch_range_scan_f16_t<false>(E, a, grid, st);
}

}  // namespace mmr
