// Labelled threshold sweep over fp16 galleries for gfx950: sweep_scan_kernel (sweep.hip) with fp16 operands.  Same body
// (sweep_scan_body.inc), same histogram and candidate list; sweep.hip's recheck reads the fp16 rows.  A translation unit of
// its own: the kernel set of sweep.hip is counted by the ISA tests.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "sweep_scan_body.h"
#include "scan_f16.h"

namespace mmr {

template <int E, bool MASKED>
__global__ __launch_bounds__(SweepCfg<E>::THREADS, SweepCfg<E>::WAVES / 4) void sweep_scan_f16_kernel(SweepScanArgs a)
{
    using ET = f16_t;
    constexpr bool QMASK = false;
    constexpr QMaskArgs qm{};
#include "sweep_scan_body.inc"
}

// launch_scan_kernel with a per-call LDS size: the limit is raised once to the most a call can ask for
template <auto K>
static int launch_sweep_f16_kernel(unsigned grid, int threads, int lds, int lds_max, hipStream_t st, const SweepScanArgs &a)
{
    ProfScope prof(MMR_PROF_SCAN, st);
    static DeviceOnce once;
    if (once.first()) {
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), lds, st, a);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_sweep_scan_f16(int E, const SweepScanArgs &a, unsigned grid, int lds, int lds_max, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        using C = SweepCfg<decltype(e)::value>;
        if (a.row_mask) return launch_sweep_f16_kernel<&sweep_scan_f16_kernel<decltype(e)::value, true>>(grid, C::THREADS, lds, lds_max, st, a);
        return launch_sweep_f16_kernel<&sweep_scan_f16_kernel<decltype(e)::value, false>>(grid, C::THREADS, lds, lds_max, st, a);
    });
}

}  // namespace mmr
