// Silhouette sums over fp16 galleries for gfx950: the fp16 instantiations of silhouette_scan_kernel
// (silhouette_scan_body.h).  Same plan, same partials.  A translation unit of its own, as the other scans' fp16 forms.
#include "silhouette_scan_body.h"

namespace mmr {

template int launch_silhouette_scan<f16_t>(int, int, const SilScanArgs &, unsigned, hipStream_t);

}  // namespace mmr
