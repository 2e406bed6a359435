// The fp16 forms of the MFMA gallery scans, as host-side launchers: the kernels live in translation units of their own
// (search_f16.hip, range_f16.hip, sweep_f16.hip, decide_f16.hip) and share their bodies with the bf16 kernels
// (topk_scan_body.h, range_scan_body.inc, sweep_scan_body.inc, decide_scan_body.inc).  An fp16 gallery has the bf16 gallery's tile layout, LDS ring, bytes and plan;
// only the MFMA instruction differs (v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x32_f16).
#pragma once
#include "mmr_common.h"
#include "topk_scan.h"

namespace mmr {

struct RangeScanArgs;
struct SweepScanArgs;
struct DecideScanArgs;
struct AssignScanArgs;

// launch_scan_bf16's twin (search.hip), same arguments: one pass of the top-k scan for Qc fp16 queries over an fp16 gallery;
// launch_topk_scan (search.hip) picks between them
int launch_scan_f16(int E, const f16_t *q, const f16_t *gal, int Qc, int64_t N, const TopkScanGeom &g, int qpad, float *bmax,
                    float *tmax, const uint32_t *row_mask, hipStream_t st);
// launch_range_scan_E's twin (range.hip); a.q / a.gal point at fp16 elements
int launch_range_scan_f16(int E, bool tri, const RangeScanArgs &a, unsigned grid, hipStream_t st);
// launch_sweep_scan_E's twin (sweep.hip) with the LDS size that function computed; lds_max: the limit to raise once
int launch_sweep_scan_f16(int E, const SweepScanArgs &a, unsigned grid, int lds, int lds_max, hipStream_t st);
// launch_decide_scan_E's twin (decide.hip); a.q / a.gal point at fp16 elements
int launch_decide_scan_f16(int E, const DecideScanArgs &a, unsigned grid, hipStream_t st);
// launch_assign_scan_E's twin (assign.hip); a.cen / a.gal point at fp16 elements
int launch_assign_scan_f16(int E, const AssignScanArgs &a, unsigned grid, hipStream_t st);

}  // namespace mmr
