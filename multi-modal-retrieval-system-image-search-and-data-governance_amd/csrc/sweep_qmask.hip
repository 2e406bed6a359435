// Labelled threshold sweep with a row mask per query for gfx950: mmr_threshold_sweep_qmasked's scan kernels (its host
// side is sweep.hip's, shared with mmr_threshold_sweep).  Same body as sweep_scan_kernel (sweep_scan_body.inc, QMASK): the
// task's mask words [tile][query] are staged in LDS beside the task's labels, and the per-row `live` test of the binning
// epilogue reads the row's query's word.  A translation unit of its own: the kernel sets of sweep.hip and sweep_f16.hip are
// counted by the ISA tests and stay as they are.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "range_common.h"
#include "sweep_scan_body.h"
#include "scan_f16.h"

namespace mmr {

template <class ET_, int E>
__global__ __launch_bounds__(SweepCfg<E>::THREADS, SweepCfg<E>::WAVES / 4) void sweep_scan_qm_kernel(SweepScanArgs a, QMaskArgs qm)
{
    using ET = ET_;
    constexpr bool MASKED = false;
    constexpr bool QMASK = true;
#include "sweep_scan_body.inc"
}

template <auto K>
static int launch_sweep_qm_kernel(unsigned grid, int threads, int lds, int lds_max, hipStream_t st, const SweepScanArgs &a,
                                  const QMaskArgs &qm)
{
    ProfScope prof(MMR_PROF_SCAN, st);
    static DeviceOnce once;
    if (once.first()) {
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), lds, st, a, qm);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_sweep_scan_qmasked(int E, bool f16, const SweepScanArgs &a, const QMaskArgs &qm, unsigned grid, int lds, int lds_max,
                              hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        constexpr int EE = decltype(e)::value;
        using C = SweepCfg<EE>;
        if (f16) return launch_sweep_qm_kernel<&sweep_scan_qm_kernel<f16_t, EE>>(grid, C::THREADS, lds, lds_max, st, a, qm);
        return launch_sweep_qm_kernel<&sweep_scan_qm_kernel<bf16_t, EE>>(grid, C::THREADS, lds, lds_max, st, a, qm);
    });
}

}  // namespace mmr
