// The exact fp32 products of the Tip-Adapter kernels (tip_train.hip, tip_grid.hip): a block of 16 feature rows held in LDS
// as fp32, multiplied with rows of a matrix in global memory by the fp32-input MFMA (16x16x4), which is bit for bit a
// k-ordered fmaf chain.  Header-only; both files get the same code.
#pragma once
#include "mmr_common.h"

namespace mmr {

constexpr int TT_BM = 16;    // batch rows per workgroup of the forward kernel
constexpr int TT_PAD = 4;    // floats of padding per row of the LDS feature block (keeps rows 16-byte aligned)
constexpr int TT_CMAX = 64;  // classes: one lane each
constexpr int TT_FU = 8;     // forward kernel: MFMA steps (16 k each) per trip of the K loop

// four consecutive elements of a row, widened exactly to fp32
template <class T>
__device__ __forceinline__ float4 tt_load4(const T *p)
{
    if constexpr (__is_same(T, float)) {
        return *reinterpret_cast<const float4 *>(p);
    } else if constexpr (__is_same(T, bf16_t)) {
        const uint2 x = *reinterpret_cast<const uint2 *>(p);
        return make_float4(__uint_as_float(x.x << 16), __uint_as_float(x.x & 0xffff0000u), __uint_as_float(x.y << 16),
                           __uint_as_float(x.y & 0xffff0000u));
    } else {
        const f16x4 x = *reinterpret_cast<const f16x4 *>(p);
        return make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
    }
}

// Loads are never made conditional in these files: a guarded load becomes a branch with a wait of its own, and the kernels
// are bound by load latency (one wave per SIMD).  An address past the end is clamped to the last row, and where the
// duplicate must not count, it is multiplied by tt_mask (0 or 1) -- a select the compiler would turn back into a branch.
__device__ __forceinline__ float tt_mask(bool in_range) { return in_range ? 1.f : 0.f; }

__device__ __forceinline__ f32x4 tt_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// D[i][j] = sum_k Fs[i][k] * X[row0 + j][k] for the 16 LDS rows i and 32 rows j of X[nrows,E] (rows past the end are
// clamped: the caller drops them).  acc0 holds j = 0..15, acc1 j = 16..31, in the 16x16 C/D layout: column j on lane & 15,
// row i = 4*(lane >> 4) + reg.  Lane (r, h) feeds k = 16*step + 4*h + c to MFMA c of a step, both operands alike.
template <class TX>
__device__ __forceinline__ void tt_rows_times_block(const float *Fs, int ldf, const TX *X, int row0, int nrows, int E,
                                                    f32x4 &acc0, f32x4 &acc1)
{
    const int lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
    const int i0 = min(row0 + r, nrows - 1), i1 = min(row0 + 16 + r, nrows - 1);
    const TX *x0 = X + (size_t)i0 * E + 4 * h, *x1 = X + (size_t)i1 * E + 4 * h;
    const float *a = Fs + r * ldf + 4 * h;
    acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
    acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    // E is a multiple of 128: TT_FU = 8 steps (32 MFMAs per accumulator) a trip.  One wave per SIMD runs here and nothing
    // else hides a load, so a trip's global operands are fetched during the trip before: a trip then costs the longer of
    // its MFMAs (about 0.85 us) and one round trip to L2
    float4 b0[TT_FU], b1[TT_FU];
#pragma unroll
    for (int u = 0; u < TT_FU; ++u) {
        b0[u] = tt_load4<TX>(x0 + 16 * u);
        b1[u] = tt_load4<TX>(x1 + 16 * u);
    }
    for (int k0 = 0; k0 < E; k0 += 16 * TT_FU) {
        const int kn = k0 + 16 * TT_FU < E ? k0 + 16 * TT_FU : k0;   // the last trip fetches itself again: nothing out of range
        float4 av[TT_FU], n0[TT_FU], n1[TT_FU];
#pragma unroll
        for (int u = 0; u < TT_FU; ++u) {
            n0[u] = tt_load4<TX>(x0 + kn + 16 * u);
            n1[u] = tt_load4<TX>(x1 + kn + 16 * u);
            av[u] = *reinterpret_cast<const float4 *>(a + k0 + 16 * u);
        }
#pragma unroll
        for (int u = 0; u < TT_FU; ++u) {
            acc0 = tt_mfma(av[u].x, b0[u].x, acc0);
            acc1 = tt_mfma(av[u].x, b1[u].x, acc1);
            acc0 = tt_mfma(av[u].y, b0[u].y, acc0);
            acc1 = tt_mfma(av[u].y, b1[u].y, acc1);
            acc0 = tt_mfma(av[u].z, b0[u].z, acc0);
            acc1 = tt_mfma(av[u].z, b1[u].z, acc1);
            acc0 = tt_mfma(av[u].w, b0[u].w, acc0);
            acc1 = tt_mfma(av[u].w, b1[u].w, acc1);
        }
#pragma unroll
        for (int u = 0; u < TT_FU; ++u) {
            b0[u] = n0[u];
            b1[u] = n1[u];
        }
    }
}

__device__ __forceinline__ float tt_readlane(float v, int j)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

}  // namespace mmr
