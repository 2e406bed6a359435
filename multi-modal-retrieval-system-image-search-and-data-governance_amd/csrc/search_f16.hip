// Top-k scans over fp16 galleries for gfx950: the fp16 instantiations of scan_kernel / scan16_kernel (topk_scan_body.h).
// Same bmax / tmax outputs, so search.hip's finalize kernels do not care which scan ran; the exact re-score reads the fp16
// rows (exact_dot.h: load_chunk_f16).  A translation unit of its own: it compiles beside search.hip, and the kernel set
// of search.hip is counted by the ISA tests.
#include "topk_scan_body.h"

namespace mmr {

template int launch_topk_scan_16<f16_t>(int, const f16_t *, const f16_t *, int, int64_t, const TopkScanGeom &, int, float *, float *,
                                        const uint32_t *, hipStream_t);

}  // namespace mmr
