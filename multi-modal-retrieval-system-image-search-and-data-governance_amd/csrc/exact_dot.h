// Exact fp64 dot products in the fixed summation order oracle/search_ref.c replicates: the helpers shared by the top-k
// re-score (search.hip, deep_topk.hip, deep_qmask.hip), the threshold rechecks (range.hip, sweep.hip, decide.hip), the
// assignment recheck (assign.hip) and the distances to a centre (cluster_rank.hip, kmeanspp.hip).
#pragma once
#include "mmr_common.h"

namespace mmr {

// ---------------------------------------------------------------------------------------------
// exact fp64 dot, shared by finalize / exhaustive / similarity
// ---------------------------------------------------------------------------------------------
// A row of E elements is 64 contiguous chunks of PER = E/64 elements.  load_chunk fetches chunk
// `c` (for a full-wave dot, c = lane).
template <int PER>
__device__ __forceinline__ void load_chunk_bf16(const bf16_t *row, int c, float (&out)[PER]) {
    const bf16_t *p = row + c * PER;
    if constexpr (PER % 8 == 0) {
#pragma unroll
        for (int v = 0; v < PER / 8; ++v) {
            bf16x8 x = *reinterpret_cast<const bf16x8 *>(p + v * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) out[v * 8 + j] = bf16_to_f32((bf16_t)x[j]);
        }
    } else if constexpr (PER % 4 == 0) {
#pragma unroll
        for (int v = 0; v < PER / 4; ++v) {
            uint2 x = *reinterpret_cast<const uint2 *>(p + v * 4);
            out[v * 4 + 0] = __uint_as_float(x.x << 16);
            out[v * 4 + 1] = __uint_as_float(x.x & 0xffff0000u);
            out[v * 4 + 2] = __uint_as_float(x.y << 16);
            out[v * 4 + 3] = __uint_as_float(x.y & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) out[j] = bf16_to_f32(p[j]);
    }
}
template <int PER>
__device__ __forceinline__ void load_chunk_f32(const float *row, int c, float (&out)[PER]) {
    const float *p = row + c * PER;
    if constexpr (PER % 4 == 0) {
#pragma unroll
        for (int v = 0; v < PER / 4; ++v) {
            float4 x = *reinterpret_cast<const float4 *>(p + v * 4);
            out[v * 4 + 0] = x.x; out[v * 4 + 1] = x.y; out[v * 4 + 2] = x.z; out[v * 4 + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) out[j] = p[j];
    }
}
// fp16 -> fp32 is exact (subnormals included: see b16_to_f32)
template <int PER>
__device__ __forceinline__ void load_chunk_f16(const f16_t *row, int c, float (&out)[PER]) {
    const f16_t *p = row + c * PER;
    if constexpr (PER % 8 == 0) {
#pragma unroll
        for (int v = 0; v < PER / 8; ++v) {
            const f16x8 x = *reinterpret_cast<const f16x8 *>(p + v * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) out[v * 8 + j] = (float)x[j];
        }
    } else if constexpr (PER % 4 == 0) {
#pragma unroll
        for (int v = 0; v < PER / 4; ++v) {
            const f16x4 x = *reinterpret_cast<const f16x4 *>(p + v * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[v * 4 + j] = (float)x[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) out[j] = (float)p[j];
    }
}
// by element type, not by size: bf16_t and f16_t are both two bytes
template <typename T, int PER>
__device__ __forceinline__ void load_chunk(const T *row, int c, float (&out)[PER]) {
    if constexpr (__is_same(T, f16_t)) load_chunk_f16<PER>(row, c, out);
    else if constexpr (__is_same(T, bf16_t)) load_chunk_bf16<PER>(row, c, out);
    else load_chunk_f32<PER>((const float *)row, c, out);
}

// One chunk's partial: PER products summed left to right from 0.0 in fp64 (products are exact).
template <int PER>
__device__ __forceinline__ double chunk_partial(const float (&qv)[PER], const float (&gv)[PER]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) acc += (double)qv[j] * (double)gv[j];
    return acc;
}

// Full-wave form: lane l owns chunk l; the 64 partials meet in an xor-butterfly (32,16,...,1):
// the order oracle/search_ref.c replicates.
template <int PER>
__device__ __forceinline__ double exact_dot(const float (&qv)[PER], const float (&gv)[PER]) {
    return wave_sum_f64_butterfly(chunk_partial<PER>(qv, gv));
}

// Quarter-wave form: 16 lanes own one row; lane m (0..15) owns chunks m, m+16, m+32, m+48.  The
// butterfly's 32- and 16-steps pair exactly those chunks, so they become in-lane adds and only
// the 8,4,2,1 steps cross lanes: bit-identical to exact_dot, four rows per wave pass.
// QuadRow: one lane's four chunks of a row whose elements are T, as fp32 -- a query and a gallery row alike.
template <typename T, int PER>
struct QuadRow {
    float v[4][PER];
    __device__ __forceinline__ void load(const T *row, int m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_chunk<T, PER>(row, m + 16 * i, v[i]);
    }
    // the same chunks of a row kept in fp32 whatever T is (a centre to dot rows of T with)
    __device__ __forceinline__ void load_f32(const float *row, int m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_chunk<float, PER>(row, m + 16 * i, v[i]);
    }
};
template <typename T, int PER>
using QuadQuery = QuadRow<T, PER>;

template <typename T, int PER>
__device__ __forceinline__ double quad_dot(const QuadRow<T, PER> &q, const QuadRow<T, PER> &g) {
    const double p0 = chunk_partial<PER>(q.v[0], g.v[0]);
    const double p1 = chunk_partial<PER>(q.v[1], g.v[1]);
    const double p2 = chunk_partial<PER>(q.v[2], g.v[2]);
    const double p3 = chunk_partial<PER>(q.v[3], g.v[3]);
    double s = (p0 + p2) + (p1 + p3);   // butterfly steps 32 then 16
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}
// the row's squared norm, in the order every dot is taken in
template <typename T, int PER>
__device__ __forceinline__ double quad_norm(const QuadRow<T, PER> &x) { return quad_dot<T, PER>(x, x); }

}  // namespace mmr
