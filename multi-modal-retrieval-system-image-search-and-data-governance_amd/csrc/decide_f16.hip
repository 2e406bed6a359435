// Decision masks over fp16 galleries for gfx950: the fp16 instantiations of decide_scan_kernel (decide_scan_body.h).
// Same candidate list; decide.hip's recheck reads the fp16 rows.  A translation unit of its own, like the other fp16
// scans.
#include "decide_scan_body.h"

namespace mmr {

template int launch_decide_scan<f16_t>(int, const DecideScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
