// Nearest-centroid assignment over fp16 galleries for gfx950: the fp16 instantiations of assign_scan_kernel
// (assign_scan_body.h).  Same triples; assign.hip's merge, recheck and score kernels serve both.  A translation unit of
// its own, like the other fp16 scans.
#include "assign_scan_body.h"

namespace mmr {

template int launch_assign_scan<f16_t>(int, const AssignScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
