// Labelled threshold sweep over fp16 galleries for gfx950: the fp16 instantiations of sweep_scan_kernel
// (sweep_scan_body.h).  Same histogram and candidate list; sweep.hip's recheck reads the fp16 rows.  A translation unit of
// its own: it compiles beside sweep.hip, and the kernel set of sweep.hip is counted by the ISA tests.
#include "sweep_scan_body.h"

namespace mmr {

template int launch_sweep_scan<f16_t>(int, const SweepScanArgs &, unsigned, int, hipStream_t);

}  // namespace mmr
