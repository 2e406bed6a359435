// Top-k scans over fp16 galleries for gfx950: scan_kernel / scan16_kernel (search.hip) with fp16 operands.  Same bodies
// (topk_scan_body.h), same bmax / tmax outputs, so search.hip's finalize kernels do not care which scan ran; the exact
// re-score reads the fp16 rows (exact_dot.h: load_chunk_f16).  A translation unit of its own: the kernel sets of
// search.hip are counted by the ISA tests.
#include "mmr_common.h"
#include "scan_pipeline.h"
#include "topk_scan_body.h"
#include "scan_f16.h"
#include "scan_host.h"

namespace mmr {

template <int E, bool MASKED>
__global__ __launch_bounds__(ScanCfg<E>::THREADS, ScanCfg<E>::WAVES / 4) void scan_f16_kernel(
    const f16_t *__restrict__ q, const f16_t *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask)
{
    scan_body<f16_t, E, MASKED>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, row_mask);
}

template <int E, bool MASKED>
__global__ __launch_bounds__(Scan16Cfg<E>::THREADS, 2) void scan16_f16_kernel(
    const f16_t *__restrict__ q, const f16_t *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt,
    int qwaves, int qpad, float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_mask)
{
    scan16_body<f16_t, E, MASKED>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, row_mask);
}

int launch_scan_f16(int E, const f16_t *q, const f16_t *gal, int Qc, int64_t N, const TopkScanGeom &g, int qpad, float *bmax,
                    float *tmax, const uint32_t *row_mask, hipStream_t st)
{
    return scan_dispatch_E(E, [&](auto e) {
        return dispatch_masked(row_mask, [&](auto m) -> int {
            constexpr int EE = decltype(e)::value;
            constexpr bool MASKED = decltype(m)::value;
            if constexpr (EE == 768)
                return launch_scan_kernel<&scan16_f16_kernel<EE, MASKED>>(g.ntasks, Scan16Cfg<EE>::THREADS, Scan16Cfg<EE>::LDS, st, q,
                                                                          gal, Qc, N, g.ntiles, g.tpt, qpad / 16, qpad, bmax, tmax,
                                                                          row_mask);
            else
                return launch_scan_kernel<&scan_f16_kernel<EE, MASKED>>(g.ntasks, ScanCfg<EE>::THREADS, ScanCfg<EE>::LDS, st, q, gal,
                                                                        Qc, N, g.ntiles, g.tpt, qpad / 32, qpad, bmax, tmax, row_mask);
        });
    });
}

}  // namespace mmr
