// Row kernels of the CLIP towers for gfx950: patch gather, embeddings (+pre-LN), LayerNorm,
// pooling LayerNorm, output cast / L2-normalise.  The attention core is attention.hip.
// Arithmetic follows SURVEY.md Appendix A (transformers/models/clip/modeling_clip.py @5.15.0):
//   embeddings :209-217,251-254   pre_layrnorm :642   post/final LN :559,650
// LayerNorm statistics and the residual stream are fp32; GEMM inputs are bf16.
#include "encoder_ops.h"

#include <math.h>

namespace mmr {

// ---------------------------------------------------------------------------------------------
// patches: pixels[B,3,S,S] -> Ap[B*G*G (padded rows untouched), Kpad] bf16, k = (c, ky, kx), zero pad
// ---------------------------------------------------------------------------------------------
template <typename TIN>
__global__ __launch_bounds__(256) void im2col_kernel(const TIN *__restrict__ px, bf16_t *__restrict__ ap, int B,
                                                     int S, int P, int G, int K, int Kpad)
{
    const int chunks_per_row = Kpad / 8;
    const int64_t total = (int64_t)B * G * G * chunks_per_row;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        const int ch = (int)(id % chunks_per_row);
        const int64_t row = id / chunks_per_row;
        const int gx = (int)(row % G), gy = (int)((row / G) % G), b = (int)(row / ((int64_t)G * G));
        float v[8];
        const int k0 = ch * 8;
        if ((P & 7) == 0 && k0 + 8 <= K) {
            // 8 consecutive kx inside one (c, ky): a contiguous pixel run
            const int c = k0 / (P * P), rem = k0 % (P * P), ky = rem / P, kx = rem % P;
            const TIN *src = px + (((size_t)b * 3 + c) * S + (gy * P + ky)) * S + gx * P + kx;
            if constexpr (sizeof(TIN) == 4) {
                const float4 a = *reinterpret_cast<const float4 *>(src);
                const float4 bq = *reinterpret_cast<const float4 *>(src + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = bq.x; v[5] = bq.y; v[6] = bq.z; v[7] = bq.w;
            } else {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(src);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32((bf16_t)a[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                float x = 0.f;
                if (k < K) {
                    const int c = k / (P * P), rem = k % (P * P), ky = rem / P, kx = rem % P;
                    const TIN *src = px + (((size_t)b * 3 + c) * S + (gy * P + ky)) * S + gx * P + kx;
                    if constexpr (sizeof(TIN) == 4) x = *src; else x = bf16_to_f32(*(const bf16_t *)src);
                }
                v[j] = x;
            }
        }
        uint4 o;
        o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
        o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4 *>(ap + (size_t)row * Kpad + k0) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// row LayerNorm helpers: one wave per row, VPL = d/64 values per lane held in registers
// ---------------------------------------------------------------------------------------------
// wave-wide sum in plain VALU: DPP inside each row of 16 lanes, then gfx950's row swaps across the four rows.
// (__shfl_xor lowers to ds_bpermute: six dependent LDS-crossbar round trips per reduction.)
__device__ __forceinline__ float wave_sum_valu(float v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    v = row16_sum(v);
    const u32x2 a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a.x) + __uint_as_float(a.y);           // .x/.y + __uint_as_float: see quad_rows_reduce (attention.hip)
    const u32x2 c = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(c.x) + __uint_as_float(c.y);
}

template <int VPL>
__device__ __forceinline__ void ln_row(float (&x)[VPL], const float *__restrict__ w, const float *__restrict__ b,
                                       int lane, int d, float eps)
{
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) s += x[j];
    const float mean = wave_sum_valu(s) / (float)d;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) { const float t = x[j] - mean; ss += t * t; }
    const float rstd = rsqrtf(wave_sum_valu(ss) / (float)d + eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int col = j * 64 + lane;
        x[j] = (x[j] - mean) * rstd * w[col] + b[col];
    }
}

// LN-fold producers (tower.hip, fold_ln): alongside h emit x = bf16(h) and the row's (sum, sumsq) in the
// partial-sum layout the GEMM epilogue reads (mmr_common.h GemmAux): slot 0 carries the row, the rest are 0.
template <int VPL>
__device__ __forceinline__ void emit_fold_inputs(const float (&x)[VPL], int lane, int64_t row, int d, bf16_t *__restrict__ xb,
                                                 float2 *__restrict__ stats)
{
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        s += x[j];
        ss += x[j] * x[j];
        xb[(size_t)row * d + j * 64 + lane] = f32_to_bf16(x[j]);
    }
    s = wave_sum_valu(s);
    ss = wave_sum_valu(ss);
    if (lane < LNFOLD_NP) stats[(size_t)row * LNFOLD_NP + lane] = lane == 0 ? make_float2(s, ss) : make_float2(0.f, 0.f);
}

// h[b*T + t] = LN_pre( (t == 0 ? cls : pe[b*G*G + t-1]) + pos[t] )        (fp32 residual stream)
template <int VPL>
__global__ __launch_bounds__(256) void embed_vision_kernel(const float *__restrict__ pe, const float *__restrict__ cls,
                                                           const float *__restrict__ pos, const float *__restrict__ lw,
                                                           const float *__restrict__ lb, float *__restrict__ h, int B,
                                                           int T, int d, float eps, bf16_t *__restrict__ xb,
                                                           float2 *__restrict__ stats, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    // the workspace's status word (include/mmr.h): nothing in a vision forward can raise a bit, so the word is zeroed
    // here instead of by a memset launch of its own (one dependent launch less on the batch-1 path)
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * T) return;
    const int t = (int)(row % T);
    const int64_t b = row / T;
    const float *src = t == 0 ? cls : pe + (size_t)(b * (T - 1) + t - 1) * d;
    float x[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) x[j] = src[j * 64 + lane] + pos[(size_t)t * d + j * 64 + lane];
    ln_row<VPL>(x, lw, lb, lane, d, eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) h[(size_t)row * d + j * 64 + lane] = x[j];
    if (xb) emit_fold_inputs<VPL>(x, lane, row, d, xb, stats);
}

// h[n*T + t] = tok[ids[n,t]] + pos[t]
template <int VPL>
__global__ __launch_bounds__(256) void embed_text_kernel(const int32_t *__restrict__ ids, const bf16_t *__restrict__ tok,
                                                         const float *__restrict__ pos, float *__restrict__ h, int Nb,
                                                         int T, int d, int vocab, bf16_t *__restrict__ xb,
                                                         float2 *__restrict__ stats, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)Nb * T) return;
    const int t = (int)(row % T);
    int id = ids[row];
    // out-of-range ids: clamped (memory guard) and reported through the workspace's status word -- the host does
    // not read ids that already live on the GPU (that would be a sync per call)
    if ((id < 0 || id >= vocab) && lane == 0) atomicOr(status, 1);
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    float x[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int col = j * 64 + lane;
        x[j] = bf16_to_f32(tok[(size_t)id * d + col]) + pos[(size_t)t * d + col];
        h[(size_t)row * d + col] = x[j];
    }
    if (xb) emit_fold_inputs<VPL>(x, lane, row, d, xb, stats);
}

// x_bf16[row] = LN(h[row]).  RPW rows per wave, all of their loads issued before the first reduction (several rounds of
// waves over the chip's 8 192 wave slots otherwise pay the load latency once per round).
template <int VPL, int RPW>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ h, const float *__restrict__ w,
                                                        const float *__restrict__ b, bf16_t *__restrict__ x, int64_t rows,
                                                        int d, float eps)
{
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    float v[RPW][VPL];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int64_t row = row0 + r < rows ? row0 + r : rows - 1;      // a ragged last wave re-reads the last row
#pragma unroll
        for (int j = 0; j < VPL; ++j) v[r][j] = h[(size_t)row * d + j * 64 + lane];
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        ln_row<VPL>(v[r], w, b, lane, d, eps);
        if (row0 + r < rows) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) x[(size_t)(row0 + r) * d + j * 64 + lane] = f32_to_bf16(v[r][j]);
        }
    }
}

// BERT embeddings (transformers/models/bert/modeling_bert.py:53-108): word[ids] + type[0] + pos[t] -> LayerNorm
// -> h (fp32) and x = bf16(h)
template <int VPL>
__global__ __launch_bounds__(256) void embed_bert_kernel(const int32_t *__restrict__ ids, const bf16_t *__restrict__ tok,
                                                         const float *__restrict__ pos, const float *__restrict__ type0,
                                                         const float *__restrict__ lw, const float *__restrict__ lb,
                                                         float *__restrict__ h, bf16_t *__restrict__ x, int Nb, int T,
                                                         int d, int vocab, float eps, const int32_t *__restrict__ types,
                                                         int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)Nb * T) return;
    const int t = (int)(row % T);
    int id = ids[row];
    int ty = types ? types[row] : 0;                       // token_type_ids (segment 0 / 1); absent = all zero
    if ((id < 0 || id >= vocab || ty < 0 || ty > 1) && lane == 0) atomicOr(status, 1);
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    ty = ty < 0 ? 0 : (ty > 1 ? 1 : ty);
    const float *typ = type0 + (size_t)ty * d;
    float v[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int col = j * 64 + lane;
        // same association as HF: (word + type) + position
        v[j] = (bf16_to_f32(tok[(size_t)id * d + col]) + typ[col]) + pos[(size_t)t * d + col];
    }
    ln_row<VPL>(v, lw, lb, lane, d, eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        h[(size_t)row * d + j * 64 + lane] = v[j];
        x[(size_t)row * d + j * 64 + lane] = f32_to_bf16(v[j]);
    }
}

// post-LN blocks (BERT): h = LN(h) in place, x = bf16(h)
template <int VPL>
__global__ __launch_bounds__(256) void layernorm_inplace_kernel(float *__restrict__ h, const float *__restrict__ w,
                                                                const float *__restrict__ b, bf16_t *__restrict__ x,
                                                                int64_t rows, int d, float eps)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = h[(size_t)row * d + j * 64 + lane];
    ln_row<VPL>(v, w, b, lane, d, eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        h[(size_t)row * d + j * 64 + lane] = v[j];
        x[(size_t)row * d + j * 64 + lane] = f32_to_bf16(v[j]);
    }
}

// xc[n] = x[n*T]  (first token of every sequence, bf16 copy for the BERT pooler)
__global__ __launch_bounds__(256) void gather_first_rows_kernel(const bf16_t *__restrict__ x, bf16_t *__restrict__ xc, int Nb,
                                                                int T, int d)
{
    const int chunks = d / 8;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= Nb * chunks) return;
    const int n = id / chunks, c = id % chunks;
    *reinterpret_cast<uint4 *>(xc + (size_t)n * d + c * 8) = *reinterpret_cast<const uint4 *>(x + (size_t)n * T * d + c * 8);
}

// pooled position of sequence n (one wave per sequence, the same value in every lane):
// vision (ids == nullptr) -> token 0; text -> first position of the largest id (EOT).
__device__ __forceinline__ int pooled_pick(const int32_t *__restrict__ ids, int n, int T, int lane)
{
    if (!ids) return 0;
    int best = -2147483647 - 1, bpos = 0;
    for (int t = lane; t < T; t += 64) {
        const int v = ids[(size_t)n * T + t];
        if (v > best) { best = v; bpos = t; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int ov = __shfl_xor(best, off, 64), op = __shfl_xor(bpos, off, 64);
        if (ov > best || (ov == best && op < bpos)) { best = ov; bpos = op; }
    }
    return bpos;
}

// xc_bf16[n] = LN(h[n*T + pooled_pick(n)])
template <int VPL>
__global__ __launch_bounds__(256) void pool_ln_kernel(const float *__restrict__ h, const int32_t *__restrict__ ids,
                                                      const float *__restrict__ w, const float *__restrict__ b,
                                                      bf16_t *__restrict__ xc, int Nb, int T, int d, float eps)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= Nb) return;
    const int pick = pooled_pick(ids, n, T, lane);
    const float *src = h + ((size_t)n * T + pick) * d;
    float v[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = src[j * 64 + lane];
    ln_row<VPL>(v, w, b, lane, d, eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) xc[(size_t)n * d + j * 64 + lane] = f32_to_bf16(v[j]);
}

// Pooled-row form of the last block (tower.hip): pick[n] = pooled_pick(n), and that row of the LN1 output and of the
// residual stream copied into compact [Nb, d] buffers: xg[n] = x[n*T + pick], hc[n] = h[n*T + pick].
template <int VPL>
__global__ __launch_bounds__(256) void pick_gather_kernel(const int32_t *__restrict__ ids, const bf16_t *__restrict__ x,
                                                          const float *__restrict__ h, bf16_t *__restrict__ xg,
                                                          float *__restrict__ hc, int32_t *__restrict__ picks, int Nb, int T,
                                                          int d)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= Nb) return;
    const int pick = pooled_pick(ids, n, T, lane);
    if (lane == 0) picks[n] = pick;
    const size_t src = ((size_t)n * T + pick) * d, dst = (size_t)n * d;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        xg[dst + j * 64 + lane] = x[src + j * 64 + lane];
        hc[dst + j * 64 + lane] = h[src + j * 64 + lane];
    }
}

// out[n] = (normalize ? f / ||f|| : f) cast to the output dtype
template <typename TOUT>
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ feat, TOUT *__restrict__ out, int Nb, int E,
                                                     int normalize)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= Nb) return;
    const float *f = feat + (size_t)n * E;
    float inv = 1.f;
    if (normalize) {
        float ss = 0.f;
        for (int j = lane; j < E; j += 64) ss += f[j] * f[j];
        inv = 1.0f / sqrtf(wave_sum(ss));
    }
    for (int j = lane; j < E; j += 64) {
        const float v = f[j] * inv;
        // by type: bf16_t is raw bits; f16_t (round-to-nearest-even, what .half() of the fp32 output gives) and float convert
        if constexpr (__is_same(TOUT, bf16_t)) out[(size_t)n * E + j] = f32_to_bf16(v);
        else out[(size_t)n * E + j] = (TOUT)v;
    }
}

// ---------------------------------------------------------------------------------------------
// launchers (internal; argument validation is done by tower.hip)
// ---------------------------------------------------------------------------------------------
#define MMR_VPL_SWITCH(d, ...)                                                     \
    switch ((d) / 64) {                                                            \
        case 2: { constexpr int VPL = 2; __VA_ARGS__; } break;                     \
        case 8: { constexpr int VPL = 8; __VA_ARGS__; } break;                     \
        case 12: { constexpr int VPL = 12; __VA_ARGS__; } break;                   \
        case 16: { constexpr int VPL = 16; __VA_ARGS__; } break;                   \
        default: set_error("width %d unsupported (128, 512, 768, 1024)", (d)); return MMR_ENOTSUP; \
    }

int launch_im2col(const void *px, mmr_dtype dt, bf16_t *ap, int B, int S, int P, int G, int K, int Kpad, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const int64_t total = (int64_t)B * G * G * (Kpad / 8);
    const unsigned blocks = grid_1d(total, 256, 8192);
    if (dt == MMR_F32) hipLaunchKernelGGL(im2col_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float *)px, ap, B, S, P, G, K, Kpad);
    else hipLaunchKernelGGL(im2col_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t *)px, ap, B, S, P, G, K, Kpad);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_embed_vision(const float *pe, const float *cls, const float *pos, const float *lw, const float *lb, float *h,
                        int B, int T, int d, float eps, bf16_t *xb, float2 *stats, int32_t *status, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)(((int64_t)B * T + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(embed_vision_kernel<VPL>, grid, dim3(256), 0, st, pe, cls, pos, lw, lb, h, B, T, d, eps, xb, stats, status));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_embed_text(const int32_t *ids, const bf16_t *tok, const float *pos, float *h, int Nb, int T, int d, int vocab,
                      bf16_t *xb, float2 *stats, int32_t *status, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)(((int64_t)Nb * T + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(embed_text_kernel<VPL>, grid, dim3(256), 0, st, ids, tok, pos, h, Nb, T, d, vocab, xb, stats, status));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_layernorm(const float *h, const float *w, const float *b, bf16_t *x, int64_t rows, int d, float eps,
                     hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    static const int force_rpw = getenv("MMR_LN_RPW") ? atoi(getenv("MMR_LN_RPW")) : 0;      // 1 / 2: A/B aid
    // measured: no change at 12 800 rows (ViT-B/32 batch 256), -6 % at 73 856 rows (ViT-L/14@336 batch 128)
    const bool two = force_rpw ? force_rpw == 2 : rows >= 32768;
    if (two) {
        const dim3 grid((unsigned)((rows + 7) / 8));
        MMR_VPL_SWITCH(d, hipLaunchKernelGGL((layernorm_kernel<VPL, 2>), grid, dim3(256), 0, st, h, w, b, x, rows, d, eps));
    } else {
        const dim3 grid((unsigned)((rows + 3) / 4));
        MMR_VPL_SWITCH(d, hipLaunchKernelGGL((layernorm_kernel<VPL, 1>), grid, dim3(256), 0, st, h, w, b, x, rows, d, eps));
    }
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_pool_ln(const float *h, const int32_t *ids, const float *w, const float *b, bf16_t *xc, int Nb, int T, int d,
                   float eps, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)((Nb + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(pool_ln_kernel<VPL>, grid, dim3(256), 0, st, h, ids, w, b, xc, Nb, T, d, eps));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_embed_bert(const int32_t *ids, const bf16_t *tok, const float *pos, const float *type0, const float *lw,
                      const float *lb, float *h, bf16_t *x, int Nb, int T, int d, int vocab, float eps, const int32_t *types,
                      int32_t *status, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)(((int64_t)Nb * T + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(embed_bert_kernel<VPL>, grid, dim3(256), 0, st, ids, tok, pos, type0, lw, lb, h, x, Nb, T, d, vocab, eps, types, status));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_layernorm_inplace(float *h, const float *w, const float *b, bf16_t *x, int64_t rows, int d, float eps,
                             hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)((rows + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(layernorm_inplace_kernel<VPL>, grid, dim3(256), 0, st, h, w, b, x, rows, d, eps));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_gather_first_rows(const bf16_t *x, bf16_t *xc, int Nb, int T, int d, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const int total = Nb * (d / 8);
    hipLaunchKernelGGL(gather_first_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, st, x, xc, Nb, T, d);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_finish(const float *feat, void *out, mmr_dtype odt, int Nb, int E, int normalize, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)((Nb + 3) / 4));
    if (odt == MMR_BF16) hipLaunchKernelGGL(finish_kernel<bf16_t>, grid, dim3(256), 0, st, feat, (bf16_t *)out, Nb, E, normalize);
    else if (odt == MMR_F16) hipLaunchKernelGGL(finish_kernel<f16_t>, grid, dim3(256), 0, st, feat, (f16_t *)out, Nb, E, normalize);
    else hipLaunchKernelGGL(finish_kernel<float>, grid, dim3(256), 0, st, feat, (float *)out, Nb, E, normalize);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

int launch_pick_gather(const int32_t *ids, const bf16_t *x, const float *h, bf16_t *xg, float *hc, int32_t *picks, int Nb, int T,
                       int d, hipStream_t st)
{
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const dim3 grid((unsigned)((Nb + 3) / 4));
    MMR_VPL_SWITCH(d, hipLaunchKernelGGL(pick_gather_kernel<VPL>, grid, dim3(256), 0, st, ids, x, h, xg, hc, picks, Nb, T, d));
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr
