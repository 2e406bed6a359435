// Nearest-centroid assignment over fp16 galleries for gfx950: assign_scan_kernel (assign.hip) with fp16 operands.  Same
// body (assign_scan_body.inc), same triples; assign.hip's merge, recheck and score kernels serve both.  A translation unit
// of its own, like the other fp16 scans.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "assign_scan_body.h"
#include "scan_f16.h"

namespace mmr {

template <int E, bool MASKED>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void assign_scan_f16_kernel(AssignScanArgs a)
{
    using ET = f16_t;
#include "assign_scan_body.inc"
}

int launch_assign_scan_f16(int E, const AssignScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        if (a.row_mask) return launch_scan_kernel<&assign_scan_f16_kernel<decltype(e)::value, true>>(grid, C::THREADS, C::LDS, st, a);
        return launch_scan_kernel<&assign_scan_f16_kernel<decltype(e)::value, false>>(grid, C::THREADS, C::LDS, st, a);
    });
}

}  // namespace mmr
