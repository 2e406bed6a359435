// Threshold search and self-join over fp16 galleries for gfx950: the fp16 instantiations of range_scan_kernel
// (range_scan_body.h).  Same candidate list; range.hip's recheck reads the fp16 rows.  A translation unit of its own: it
// compiles beside range.hip, and the kernel set of range.hip is counted by the ISA tests.
#include "range_scan_body.h"

namespace mmr {

template int launch_range_scan<f16_t>(int, bool, const RangeScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
