// Tip-Adapter (beta, alpha) grid search (reference code/utils.py:159-206 `search_hp`, with `find_thresholds`,
// `eval_threshold`, `get_similarity` of code/main_custom.py:27-105 and `cls_f1`, `cls_acc` of code/utils.py:15-76).
//
// Stage 1, floating point, computed once and returned:
//   A = F K (never written)   L0 = 100 F Wc [N,C]   cache[b] = 10 * sum_s exp(beta_b A[:,s] - beta_b) V[s,:] [nb,N,C]
// Stage 2, exact: the logit of grid point (b, a) is DEFINED as fl32(L0 + fl32(cache[b] * alpha_a)) -- one rounded multiply,
// one rounded add -- and every count, threshold and F1 is a function of those fp32 values widened to fp64.
//
// Three launches, no float atomics, nothing depends on scheduling:
//   tip_grid_cache_kernel   one workgroup owns TT_BM = 16 rows for the whole of S and every gridDim.y-th group of TG_BB
//                           betas (a small N leaves CUs idle otherwise; a slice recomputes the affinities, which cost about
//                           as much as one group of betas).  The feature block sits in LDS as fp32;
//                           S is walked in chunks of at most TG_SC columns whose 16 x chunk affinities (the exact
//                           fp32-input MFMA of tip_mfma.h) stay in LDS; per beta, exp and then P V with lane = class and s
//                           ascending.  Between chunks the running sums rest in `cache` itself (the workgroup's own rows,
//                           exact fp32), so the fmaf chain of a (b, n, c) is one chain whatever the chunking.
//   tip_grid_conf_kernel    one workgroup per (b, a): rows strided over threads, row arg-max (lowest class at the maximum),
//                           int32 counters [C,C] in LDS.
//   tip_grid_f1_kernel      one workgroup per (b, a, c): extents of pos / neg, then each row's logit is binned by the number
//                           of thresholds t_i <= x -- a guess from (x - lo) / step corrected against the exact fp64 t_i --
//                           into two LDS histograms, a suffix sum turns them into tp_i / fp_i, and the F1 arg-best (the
//                           first index at the maximum) is taken in fp64.
// This file is compiled with -ffp-contract=off (build.py): t_i = fl(fl(i * step) + lo) and the two rounded logit operations
// must not fuse, and the __f*_rn / __d*_rn intrinsics are plain operators in this toolchain's headers.
#include "mmr_common.h"
#include "scan_host.h"
#include "tip_mfma.h"

#include <math.h>
#include <algorithm>

namespace mmr {

constexpr int TG_SC = 1024;                         // columns of S per chunk of the cache kernel (a multiple of 64)
constexpr int TG_BB = 4;                            // betas per pass over a chunk: one load of V serves all of them (a float4)
static_assert(TG_BB == 4, "the cache kernel moves a row's TG_BB values of P as one float4");
constexpr int TG_NT = 512;                          // threads of the threshold-F1 kernel
constexpr int TG_BINS = MMR_TIP_GRID_MAX_VALS + 1;  // bins per histogram: a row falls into bin #{i : t_i <= x} in [0, num_vals]

static inline int tg_chunk_cols(int S) { return S < TG_SC ? (S + 63) / 64 * 64 : TG_SC; }
// LDS of the cache kernel: Fs[TT_BM][E + TT_PAD], As[TT_BM][chunk + TT_PAD], P[4 waves][64][4 rows][TG_BB]
static inline size_t tg_cache_lds(int E, int S)
{
    return ((size_t)TT_BM * (E + TT_PAD + tg_chunk_cols(S) + TT_PAD) + 4 * 64 * 4 * TG_BB) * sizeof(float);
}

template <class T, class TK>
__global__ __launch_bounds__(256) void tip_grid_cache_kernel(const T *__restrict__ f, const T *__restrict__ wct,
                                                              const TK *__restrict__ keys, const float *__restrict__ V,
                                                              const float *__restrict__ betas, int64_t N, int E, int C, int S,
                                                              int nb, int chunk, float *__restrict__ L0, float *cache)
{
    extern __shared__ float4 tg_smem[];
    const int ldf = E + TT_PAD, lda = chunk + TT_PAD;
    float *Fs = reinterpret_cast<float *>(tg_smem);
    float *As = Fs + TT_BM * ldf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    float *Pw = As + TT_BM * lda + wave * (64 * 4 * TG_BB);   // this wave's slab of P
    const int64_t n0 = (int64_t)blockIdx.x * TT_BM;

    // the feature block as fp32; rows past N repeat the last row: what is computed for them is never stored
    const int e4 = E / 4;
    for (int i = tid; i < TT_BM * e4; i += 256) {
        const int row = i / e4, c4 = i - row * e4;
        *reinterpret_cast<float4 *>(Fs + row * ldf + 4 * c4) = tt_load4<T>(f + (size_t)min(n0 + row, N - 1) * E + 4 * c4);
    }
    __syncthreads();

    // the classifier columns, 100 F Wc, straight from the accumulators to L0 (the first beta slice's workgroups only)
    for (int c0 = blockIdx.y == 0 ? wave * 32 : C; c0 < C; c0 += 128) {
        f32x4 acc[2];
        tt_rows_times_block<T>(Fs, ldf, wct, c0, C, E, acc[0], acc[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + 16 * j + r;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t n = n0 + 4 * h + reg;
                if (c < C && n < N) L0[(size_t)n * C + c] = 100.f * acc[j][reg];
            }
        }
    }

    const int cl = min(lane, C - 1);          // lanes past C compute a duplicate of class C-1 that nobody stores
    for (int cs = 0; cs < S; cs += chunk) {
        const int ce = min(cs + chunk, S);
        __syncthreads();                      // the chunk before has been consumed
        // affinities of the chunk: wave w takes the blocks of 32 columns w, w+4, ...
        for (int s0 = cs + wave * 32; s0 < ce; s0 += 128) {
            f32x4 acc[2];
            tt_rows_times_block<TK>(Fs, ldf, keys, s0, S, E, acc[0], acc[1]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int s = s0 + 16 * j + r;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (s < ce) As[(4 * h + reg) * lda + (s - cs)] = acc[j][reg];
            }
        }
        __syncthreads();

        // P V: wave w owns rows 4w..4w+3, lane c owns class c; s ascending, one fmaf chain per (beta, row, class)
        for (int bb = blockIdx.y * TG_BB; bb < nb; bb += gridDim.y * TG_BB) {
            float beta[TG_BB], pv[TG_BB][4];
#pragma unroll
            for (int q = 0; q < TG_BB; ++q) {
                const int b = min(bb + q, nb - 1);
                beta[q] = betas[b];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t n = min(n0 + 4 * wave + i, N - 1);
                    pv[q][i] = cs == 0 ? 0.f : cache[((size_t)b * N + n) * C + cl];
                }
            }
            for (int sb = cs; sb < ce; sb += 64) {
                // lane j computes the 4 x TG_BB values of P for column sb + j and parks them in the wave's slab of LDS; every
                // lane then reads them back as broadcasts, j ascending.  (Handing them round with v_readlane needs
                // 64 * 4 * TG_BB scalar registers at once.)  Past the chunk's end P is zero and the fmaf leaves pv as it is
                const bool in = sb + lane < ce;
                float p[4][TG_BB];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = As[(4 * wave + i) * lda + min(sb + lane, ce - 1) - cs];
#pragma unroll
                    for (int q = 0; q < TG_BB; ++q) p[i][q] = in ? expf(beta[q] * a - beta[q]) : 0.f;
                }
                __builtin_amdgcn_wave_barrier();          // the reads of the block before are done (LDS runs a wave in order)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<float4 *>(Pw + lane * (4 * TG_BB) + i * TG_BB) = make_float4(p[i][0], p[i][1], p[i][2], p[i][3]);
                __builtin_amdgcn_wave_barrier();
                // the loads of V are all in flight at once
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    const float v = V[(size_t)min(sb + j, S - 1) * C + cl];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 pj = *reinterpret_cast<const float4 *>(Pw + j * (4 * TG_BB) + i * TG_BB);
                        pv[0][i] = fmaf(pj.x, v, pv[0][i]);
                        pv[1][i] = fmaf(pj.y, v, pv[1][i]);
                        pv[2][i] = fmaf(pj.z, v, pv[2][i]);
                        pv[3][i] = fmaf(pj.w, v, pv[3][i]);
                    }
                }
            }
            const float scale = ce == S ? 10.f : 1.f;      // the running sum rests unscaled until the last chunk
#pragma unroll
            for (int q = 0; q < TG_BB; ++q) {
                const int b = bb + q;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t n = n0 + 4 * wave + i;
                    if (b < nb && n < N && lane < C) cache[((size_t)b * N + n) * C + lane] = scale * pv[q][i];
                }
            }
        }
    }
}

// the logit of a grid point: one rounded multiply, one rounded add (never contracted: see the file's flag)
__device__ __forceinline__ float tg_logit(float l0, float cache, float alpha) { return __fadd_rn(l0, __fmul_rn(cache, alpha)); }

__global__ __launch_bounds__(256) void tip_grid_conf_kernel(const float *__restrict__ L0, const float *__restrict__ cache,
                                                             const int64_t *__restrict__ y, const float *__restrict__ alphas,
                                                             int64_t N, int C, int na, int32_t *__restrict__ conf,
                                                             int32_t *__restrict__ status)
{
    __shared__ int32_t cnt[TT_CMAX * TT_CMAX];
    const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < C * C; i += 256) cnt[i] = 0;
    __syncthreads();
    const float alpha = alphas[a];
    const float *cb = cache + (size_t)b * N * C;
    bool bad = false;
    for (int64_t n = tid; n < N; n += 256) {
        const int64_t t = y[n];
        if (t < 0 || t >= C) {
            bad = true;
            continue;
        }
        const float *l0 = L0 + (size_t)n * C, *cr = cb + (size_t)n * C;
        float best = tg_logit(l0[0], cr[0], alpha);
        int pred = 0;
        for (int c = 1; c < C; ++c) {
            const float x = tg_logit(l0[c], cr[c], alpha);
            if (x > best) {
                best = x;
                pred = c;
            }
        }
        atomicAdd(&cnt[(int)t * C + pred], 1);
    }
    // an idempotent integer OR, as in the training step; every workgroup sees the same labels, so one of them reports
    if (bad && a == 0 && b == 0) atomicOr(status, 1);
    __syncthreads();
    int32_t *out = conf + ((size_t)b * na + a) * C * C;
    for (int i = tid; i < C * C; i += 256) out[i] = cnt[i];
}

// t_i of np.linspace(lo, hi, nv) in fp64: fl(fl(i * step) + lo), the last one hi itself; nv == 1 gives [fl(0 + lo)]
__device__ __forceinline__ double tg_threshold(int i, int nv, double lo, double hi, double step)
{
    if (nv == 1) return __dadd_rn(0.0, lo);
    if (i == nv - 1) return hi;
    return __dadd_rn(__dmul_rn((double)i, step), lo);
}

__global__ __launch_bounds__(TG_NT) void tip_grid_f1_kernel(const float *__restrict__ L0, const float *__restrict__ cache,
                                                             const int64_t *__restrict__ y, const float *__restrict__ alphas,
                                                             int64_t N, int C, int na, double *__restrict__ f1,
                                                             double *__restrict__ threshold, int32_t *__restrict__ tp,
                                                             int32_t *__restrict__ fp, int32_t *__restrict__ fn,
                                                             int32_t *__restrict__ num_vals, int32_t *__restrict__ status)
{
    extern __shared__ int32_t tg_hist[];       // histP[TG_BINS], histN[TG_BINS]
    constexpr int NW = TG_NT / 64;
    __shared__ float ext[4][NW];
    __shared__ int32_t cntw[2][NW];
    __shared__ int32_t part[2][TG_NT];
    __shared__ double bestf[NW];
    __shared__ int32_t besti[NW];
    int32_t *histP = tg_hist, *histN = tg_hist + TG_BINS;
    const int c = blockIdx.x, a = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float alpha = alphas[a];
    const float *l0 = L0 + c, *cr = cache + (size_t)b * N * C + c;
    const size_t at = ((size_t)b * na + a) * C + c;

    // pass 1: extents and sizes of pos (label == c) and neg (any other valid label)
    float mnP = __builtin_inff(), mxP = -__builtin_inff(), mnN = __builtin_inff(), mxN = -__builtin_inff();
    int nP = 0, nN = 0;
    for (int64_t n = tid; n < N; n += TG_NT) {
        const int64_t t = y[n];
        if (t < 0 || t >= C) continue;
        const float x = tg_logit(l0[(size_t)n * C], cr[(size_t)n * C], alpha);
        if (t == c) {
            mnP = fminf(mnP, x);
            mxP = fmaxf(mxP, x);
            ++nP;
        } else {
            mnN = fminf(mnN, x);
            mxN = fmaxf(mxN, x);
            ++nN;
        }
    }
    mnP = wave_min(mnP);
    mxP = wave_max(mxP);
    mnN = wave_min(mnN);
    mxN = wave_max(mxN);
    nP = wave_sum(nP);
    nN = wave_sum(nN);
    if (lane == 0) {
        ext[0][wave] = mnP;
        ext[1][wave] = mxP;
        ext[2][wave] = mnN;
        ext[3][wave] = mxN;
        cntw[0][wave] = nP;
        cntw[1][wave] = nN;
    }
    __syncthreads();
    mnP = ext[0][0], mxP = ext[1][0], mnN = ext[2][0], mxN = ext[3][0], nP = cntw[0][0], nN = cntw[1][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        mnP = fminf(mnP, ext[0][w]);
        mxP = fmaxf(mxP, ext[1][w]);
        mnN = fminf(mnN, ext[2][w]);
        mxN = fmaxf(mxN, ext[3][w]);
        nP += cntw[0][w];
        nN += cntw[1][w];
    }

    // every thread derives the same lo, hi, num_vals and step from the same values
    const double lo = (double)fmaxf(mnP, mnN), hi = (double)fminf(mxP, mxN);
    int nv = -1;
    if (nP > 0 && nN > 0) {
        const double d = __dmul_rn(__dsub_rn(hi, lo), 10.0);
        nv = !(d < 2147483647.0) ? 0x7fffffff : d <= -2147483648.0 ? (int)0x80000000 : (int)d;   // int(): towards zero
    }
    if (nv <= 0 || nv > MMR_TIP_GRID_MAX_VALS) {
        // degenerate: all zero.  Past the cap: NaN, never a wrong number, and bit 1 of the status word
        if (tid == 0) {
            const bool over = nv > 0;
            f1[at] = over ? __builtin_nan("") : 0.0;
            threshold[at] = over ? __builtin_nan("") : 0.0;
            tp[at] = fp[at] = fn[at] = 0;
            num_vals[at] = nv;
            if (over) atomicOr(status, 2);
        }
        return;
    }
    const int nbins = nv + 1;
    for (int i = tid; i < nbins; i += TG_NT) histP[i] = histN[i] = 0;
    __syncthreads();
    const double step = nv > 1 ? (hi - lo) / (double)(nv - 1) : 0.0;

    // pass 2: bin j = #{i : t_i <= x}.  The t_i are non-decreasing (rounding is monotone), so the guess is corrected until
    // t_{j-1} <= x < t_j
    for (int64_t n = tid; n < N; n += TG_NT) {
        const int64_t t = y[n];
        if (t < 0 || t >= C) continue;
        const double x = (double)tg_logit(l0[(size_t)n * C], cr[(size_t)n * C], alpha);
        int j;
        if (!(x >= lo)) {
            j = 0;                              // t_0 == lo
        } else if (nv == 1) {
            j = 1;
        } else {
            const double g = (x - lo) / step;
            j = g >= (double)nv ? nv : (int)g + 1;              // x >= lo: at least t_0 counts
            while (j > 1 && tg_threshold(j - 1, nv, lo, hi, step) > x) --j;
            while (j < nv && tg_threshold(j, nv, lo, hi, step) <= x) ++j;
        }
        atomicAdd(t == c ? &histP[j] : &histN[j], 1);
    }
    __syncthreads();

    // suffix sums in place: hist[j] becomes #{rows with bin >= j}, so tp_i = histP[i + 1], fp_i = histN[i + 1]
    const int per = (nbins + TG_NT - 1) / TG_NT, j0 = min(tid * per, nbins), j1 = min(j0 + per, nbins);
    int sP = 0, sN = 0;
    for (int j = j0; j < j1; ++j) {
        sP += histP[j];
        sN += histN[j];
    }
    part[0][tid] = sP;
    part[1][tid] = sN;
    __syncthreads();
    const int used = (nbins + per - 1) / per;   // threads with a range of their own
    sP = sN = 0;
    for (int k = tid + 1; k < used; ++k) {
        sP += part[0][k];
        sN += part[1][k];
    }
    for (int j = j1 - 1; j >= j0; --j) {
        sP += histP[j];
        sN += histN[j];
        histP[j] = sP;
        histN[j] = sN;
    }
    __syncthreads();

    // F1 of every threshold in fp64; the reference keeps the first f1 strictly above all earlier ones, starting from 0.0:
    // the first index at the maximum, if the maximum is above 0.  0/0 is NaN and never wins
    double bf = 0.0;
    int bi = 0x7fffffff;
    for (int i = j0; i < min(j1, nv); ++i) {
        const double tpi = (double)histP[i + 1], fpi = (double)histN[i + 1];
        const double p = tpi / (tpi + fpi), r = tpi / (double)nP;      // tp + fn = #pos
        const double f = __dmul_rn(__dmul_rn(2.0, p), r) / __dadd_rn(p, r);
        if (f > bf) {
            bf = f;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double of = __shfl_xor(bf, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (of > bf || (of == bf && oi < bi)) {
            bf = of;
            bi = oi;
        }
    }
    if (lane == 0) {
        bestf[wave] = bf;
        besti[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w)
            if (bestf[w] > bf || (bestf[w] == bf && besti[w] < bi)) {
                bf = bestf[w];
                bi = besti[w];
            }
        const bool none = bi == 0x7fffffff;
        const int tpb = none ? 0 : histP[bi + 1];
        f1[at] = none ? 0.0 : bf;
        threshold[at] = none ? 0.0 : tg_threshold(bi, nv, lo, hi, step);
        tp[at] = tpb;
        fp[at] = none ? 0 : histN[bi + 1];
        fn[at] = none ? 0 : nP - tpb;
        num_vals[at] = nv;
    }
}

template <class T, class TK>
static int tg_launch_cache(const void *features, const void *wct, const void *keys, const float *V, const float *betas,
                           int64_t N, int E, int C, int S, int nb, float *L0, float *cache, hipStream_t st)
{
    static DeviceOnce once;
    if (once.first())
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&tip_grid_cache_kernel<T, TK>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)tg_cache_lds(1024, TG_SC)));
    // beta slices: as many as keep the launch within about eight workgroups per CU of a 256-CU device.  The split changes
    // which workgroup runs a (beta, row, class) chain, never the chain
    const unsigned gx = (unsigned)((N + TT_BM - 1) / TT_BM), groups = (unsigned)((nb + TG_BB - 1) / TG_BB);
    const unsigned gy = grid_cap(std::min(groups, std::max(1u, 2048u / gx)));
    hipLaunchKernelGGL((tip_grid_cache_kernel<T, TK>), dim3(gx, gy), dim3(256), tg_cache_lds(E, S),
                       st, (const T *)features, (const T *)wct, (const TK *)keys, V, betas, N, E, C, S, nb, tg_chunk_cols(S), L0,
                       cache);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_tip_adapter_grid_workspace_bytes(int64_t N, int E, int C, int S, int nb, int na)
{
    (void)N, (void)E, (void)C, (void)S, (void)nb, (void)na;
    return 0;   // the affinities stay in LDS and the running sums rest in `cache`: nothing else is needed
}

extern "C" int mmr_tip_adapter_grid(const void *features, const int64_t *labels, mmr_dtype dtype, int64_t N, int E, int C, int S,
                                    const void *clip_weights_t, const void *keys_t, mmr_dtype keys_dtype,
                                    const float *cache_values, const float *betas, int nb, const float *alphas, int na, float *L0,
                                    float *cache, int32_t *conf, double *f1, double *threshold, int32_t *tp, int32_t *fp,
                                    int32_t *fn, int32_t *num_vals, int32_t *status, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    const EntryCheck chk{"mmr_tip_adapter_grid"};
    (void)workspace, (void)workspace_bytes;
    MMR_TRY(chk.dtype(dtype));
    MMR_CHECK_ARG(keys_dtype == dtype || keys_dtype == MMR_F32,
                  "mmr_tip_adapter_grid: keys_dtype %d must be the features' dtype %d or MMR_F32 (a TipAdapterF master weight)",
                  (int)keys_dtype, (int)dtype);
    MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff && C >= 1 && C <= TT_CMAX && S >= 1 && S <= 16384,
                  "mmr_tip_adapter_grid: bad shape N=%lld C=%d S=%d (N < 2^31-1, 1 <= C <= 64, 1 <= S <= 16384)", (long long)N, C,
                  S);
    MMR_CHECK_ARG(nb >= 0 && nb <= 65535 && na >= 0 && na <= 65535, "mmr_tip_adapter_grid: bad grid nb=%d na=%d (at most 65535 each)",
                  nb, na);
    MMR_TRY(dispatch_per(E, [](auto) -> int { return MMR_OK; }));
    if (nb == 0 || na == 0) return MMR_OK;
    MMR_CHECK_ARG(betas && alphas && conf && f1 && threshold && tp && fp && fn && num_vals && status &&
                      (N == 0 || (features && labels && clip_weights_t && keys_t && cache_values && L0 && cache)),
                  "mmr_tip_adapter_grid: null pointer");
    MMR_TRY(chk.aligned16((uintptr_t)features | (uintptr_t)clip_weights_t | (uintptr_t)keys_t, "operands"));
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        const bool f32_keys = keys_dtype == MMR_F32;
        MMR_TRY(dispatch_elem(dtype, [&](auto tag) -> int {
            using T = typename decltype(tag)::type;
            if (f32_keys)
                return tg_launch_cache<T, float>(features, clip_weights_t, keys_t, cache_values, betas, N, E, C, S, nb, L0, cache, st);
            return tg_launch_cache<T, T>(features, clip_weights_t, keys_t, cache_values, betas, N, E, C, S, nb, L0, cache, st);
        }));
    }
    hipLaunchKernelGGL(tip_grid_conf_kernel, dim3(na, nb), dim3(256), 0, st, (const float *)L0, (const float *)cache, labels,
                       alphas, N, C, na, conf, status);
    MMR_CHECK_LAUNCH();
    static DeviceOnce once;
    const size_t hist_bytes = 2 * (size_t)TG_BINS * sizeof(int32_t);
    if (once.first())
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&tip_grid_f1_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_bytes));
    hipLaunchKernelGGL(tip_grid_f1_kernel, dim3(C, na, nb), dim3(TG_NT), hist_bytes, st, (const float *)L0, (const float *)cache,
                       labels, alphas, N, C, na, f1, threshold, tp, fp, fn, num_vals, status);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
