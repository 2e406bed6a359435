// Labelled threshold sweep with a row mask per query for gfx950: mmr_threshold_sweep_qmasked's scan kernels (its host
// side is sweep.hip's, shared with mmr_threshold_sweep).  They are sweep_scan_kernel (sweep_scan_body.h) with QMaskArgs
// as a second argument: the task's mask words [tile][query] are staged in LDS beside the task's labels, and the per-row
// `live` test of the binning epilogue reads the row's query's word.  A translation unit of its own: the kernel sets of
// sweep.hip and sweep_f16.hip are counted by the ISA tests and stay as they are.
#include "sweep_scan_body.h"

namespace mmr {

int launch_sweep_scan_qmasked(int E, bool f16, const SweepScanArgs &a, const QMaskArgs &qm, unsigned grid, int lds, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        constexpr int EE = decltype(e)::value;
        using C = SweepCfg<EE>;
        if (f16) return launch_scan_kernel_lds<&sweep_scan_kernel<f16_t, EE, false, QMaskArgs>>(grid, C::THREADS, lds, SWEEP_LDS_MAX, st, a, qm);
        return launch_scan_kernel_lds<&sweep_scan_kernel<bf16_t, EE, false, QMaskArgs>>(grid, C::THREADS, lds, SWEEP_LDS_MAX, st, a, qm);
    });
}

}  // namespace mmr
