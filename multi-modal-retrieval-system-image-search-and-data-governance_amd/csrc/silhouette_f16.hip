// Silhouette sums over fp16 galleries for gfx950: silhouette_scan_kernel (silhouette.hip) with fp16 operands.  Same body
// (silhouette_scan_body.inc), same plan, same partials.  A translation unit of its own, as the other scans' fp16 forms.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "silhouette_scan_body.h"

namespace mmr {

template <int E, bool COS>
__global__ __launch_bounds__(RangeCfg<E>::THREADS, RangeCfg<E>::WAVES / 4) void silhouette_scan_f16_kernel(SilScanArgs a)
{
    using ET = f16_t;
#include "silhouette_scan_body.inc"
}

int launch_silhouette_scan_f16(int E, int metric, const SilScanArgs &a, unsigned grid, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = RangeCfg<decltype(e)::value>;
        constexpr int lds = C::LDS + SIL_NORM_LDS;
        if (metric) return launch_scan_kernel<&silhouette_scan_f16_kernel<decltype(e)::value, true>>(grid, C::THREADS, lds, st, a);
        return launch_scan_kernel<&silhouette_scan_f16_kernel<decltype(e)::value, false>>(grid, C::THREADS, lds, st, a);
    });
}

}  // namespace mmr
