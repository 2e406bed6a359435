// fp64 -> fp32 with a directed rounding: the thresholds the scans compare approximate dots with are rounded outward, so
// a comparison in fp32 never decides a pair the fp64 bound leaves open.  Used by the threshold sweep (sweep_scan_body.h)
// and the decision masks (decide_scan_body.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmr {

// (float)x rounded toward -inf / +inf
__device__ __forceinline__ float f32_down(double x)
{
    float f = (float)x;
    if ((double)f > x) {
        const uint32_t b = __float_as_uint(f);
        f = f > 0.f ? __uint_as_float(b - 1) : (f == 0.f ? __uint_as_float(0x80000001u) : __uint_as_float(b + 1));
    }
    return f;
}
__device__ __forceinline__ float f32_up(double x)
{
    float f = (float)x;
    if ((double)f < x) {
        const uint32_t b = __float_as_uint(f);
        f = f < 0.f ? __uint_as_float(b - 1) : (f == 0.f ? __uint_as_float(0x00000001u) : __uint_as_float(b + 1));
    }
    return f;
}

}  // namespace mmr
