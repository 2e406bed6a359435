// Crop descriptors, the layout of the device-built coefficient tables, and the arithmetic of one table row
// (Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter, as preprocess.resample_tables restates it).
// Shared by augment.hip (builds the tables) and preprocess.hip (applies them to the crops).
//
// The row arithmetic is one sequence of IEEE double operations, each rounded to nearest and none fused: that is what
// CPython and Pillow's C execute, so the integers that come out are theirs.  It is written once, for the device (the
// __d*_rn intrinsics) and for a host compiler (plain operators; build host code that includes this with -ffp-contract=off).
// On this toolchain the intrinsics are inline `x * y` / `x + y`, which the device compiler's default -ffp-contract=fast may
// fuse: build.py compiles augment.hip with -ffp-contract=off, and that flag is what the exactness rests on.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MMR_HD __host__ __device__ __forceinline__
#else
#define MMR_HD static inline
#endif

namespace mmr {

struct CropDesc {           // mirrors mmr_crop_desc in include/mmr.h
    const uint8_t *img;     // uint8 RGB [H,W,3] source; many crops may name one source
    int64_t tmp_off;        // byte offset of this crop's [ch,S,3] intermediate rows in the scratch, a multiple of 16
    int32_t H, W, top, left, ch, cw, flip, reserved;
};

constexpr int AUG_PRECISION_BITS = 32 - 8 - 2;        // Pillow Resample.c
constexpr int AUG_IN_MAX = 1 << 20;                   // longest crop side the tables are built for

#if defined(__HIP_DEVICE_COMPILE__)
MMR_HD double aug_add(double x, double y) { return __dadd_rn(x, y); }
MMR_HD double aug_sub(double x, double y) { return __dsub_rn(x, y); }
MMR_HD double aug_mul(double x, double y) { return __dmul_rn(x, y); }
MMR_HD double aug_div(double x, double y) { return __ddiv_rn(x, y); }
#else
MMR_HD double aug_add(double x, double y) { return x + y; }
MMR_HD double aug_sub(double x, double y) { return x - y; }
MMR_HD double aug_mul(double x, double y) { return x * y; }
MMR_HD double aug_div(double x, double y) { return x / y; }
#endif

// tables: [B][2][S] int2 bounds (axis 0 = horizontal, 1 = vertical), then [B][2][S][kmax] int32 coefficients.  Both blocks
// start 16-byte aligned when `tables` is (B * 2 * S * 8 is a multiple of 16) and every coefficient row is, as kmax % 4 == 0.
MMR_HD size_t aug_tables_bytes(int B, int S, int kmax) { return (size_t)B * 2 * S * (8 + 4 * (size_t)kmax); }
MMR_HD const int32_t *aug_bounds(const void *tables, int b, int axis, int S)
{
    return reinterpret_cast<const int32_t *>(tables) + ((size_t)b * 2 + axis) * S * 2;
}
MMR_HD const int32_t *aug_coeffs(const void *tables, int B, int b, int axis, int S, int kmax)
{
    return reinterpret_cast<const int32_t *>(tables) + (size_t)B * 2 * S * 2 + ((size_t)b * 2 + axis) * S * (size_t)kmax;
}

// (double)(in1 - in0) / outSize with the box held in fp32, as Pillow and resample_tables compute `scale`
MMR_HD double aug_scale(int in, int S) { return aug_div((double)(float)in, (double)S); }
// Pillow's ksize of a full-box bicubic resize in -> S
MMR_HD int aug_ksize(int in, int S)
{
    const double scale = aug_scale(in, S);
    const double support = aug_mul(2.0, scale < 1.0 ? 1.0 : scale);
    int c = (int)support;                              // ceil of a positive double within int range
    if ((double)c < support) ++c;
    return c * 2 + 1;
}

// what a crop must satisfy before any kernel touches memory on its behalf; a crop that fails is skipped by every kernel
MMR_HD bool aug_crop_ok(const CropDesc &d, int S, int kmax, int max_ch, int max_cw, size_t scratch_bytes)
{
    if (!d.img || d.H < 1 || d.W < 1 || d.ch < 1 || d.cw < 1 || d.top < 0 || d.left < 0) return false;
    if (d.ch > AUG_IN_MAX || d.cw > AUG_IN_MAX || d.ch > max_ch || d.cw > max_cw) return false;
    if ((int64_t)d.top + d.ch > d.H || (int64_t)d.left + d.cw > d.W) return false;
    if (aug_ksize(d.ch, S) > kmax || aug_ksize(d.cw, S) > kmax) return false;
    if (d.tmp_off < 0 || (d.tmp_off & 15)) return false;
    return (size_t)d.tmp_off + (size_t)d.ch * S * 3 + 16 <= scratch_bytes;
}

MMR_HD double aug_bicubic(double x)
{
    const double a = -0.5;                             // Pillow's bicubic_filter
    if (x < 0.0) x = -x;
    if (x < 1.0) return aug_add(aug_mul(aug_mul(aug_sub(aug_mul(a + 2.0, x), a + 3.0), x), x), 1.0);
    if (x < 2.0) return aug_mul(aug_sub(aug_mul(aug_add(aug_mul(aug_sub(x, 5.0), x), 8.0), x), 4.0), a);
    return 0.0;
}

// output coordinate xx of the full-box resize in -> S: bound = (first input index, taps), coeffs[0, kmax) with zeros
// behind the taps.  Needs aug_ksize(in, S) <= kmax.
MMR_HD void aug_table_row(int in, int S, int xx, int kmax, int32_t *bound, int32_t *coeffs)
{
    const double scale = aug_scale(in, S);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = aug_mul(2.0, filterscale);
    const double ss = aug_div(1.0, filterscale);
    const double center = aug_mul(aug_add((double)xx, 0.5), scale);
    int xmin = (int)aug_add(aug_sub(center, support), 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)aug_add(aug_add(center, support), 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > kmax) xmax = kmax;                      // cannot happen under the precondition; keeps the row in bounds
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x)                     // summed in tap order
        ww = aug_add(ww, aug_bicubic(aug_mul(aug_add(aug_sub((double)(x + xmin), center), 0.5), ss)));
    for (int x = 0; x < xmax; ++x) {
        double w = aug_bicubic(aug_mul(aug_add(aug_sub((double)(x + xmin), center), 0.5), ss));
        if (ww != 0.0) w = aug_div(w, ww);
        const double f = aug_mul(w, (double)(1 << AUG_PRECISION_BITS));
        coeffs[x] = w < 0.0 ? (int32_t)aug_add(-0.5, f) : (int32_t)aug_add(0.5, f);
    }
    for (int x = xmax; x < kmax; ++x) coeffs[x] = 0;
    bound[0] = xmin;
    bound[1] = xmax;
}

}  // namespace mmr
