// Tip-Adapter-F: one training step of the learnable cache keys on the device (reference code/main_custom.py:148-190).
//
//   A = F W^T [B,S]   P = exp(beta*A - beta)   L = 100 F Wc + 10 alpha P V [B,C]   loss = mean_b(logsumexp(L_b) - L_b[y_b])
//   G = (softmax(L) - onehot(y)) / B           dA = beta P (10 alpha G V^T)         g = dA^T F [S,E]       then AdamW on W
//
// Two launches per step, no atomics on floats, every sum in a fixed order:
//   tip_train_forward_kernel   one workgroup owns TT_BM = 16 rows of the batch for the whole of S.  The feature block sits
//                              in LDS as fp32; each wave walks S in chunks of 32 columns with the exact fp32-input MFMA
//                              (16x16x4, two independent accumulators), parks P in the workspace, then the workgroup forms
//                              P V, the classifier columns (the same MFMA routine), the max-subtracted softmax, loss_b,
//                              pred_b and G, and turns its own rows of P into dA in place.
//   tip_train_update_kernel    one wave per 16 x 64 tile of [S,E]: g = dA^T F by the same MFMA with K = B walked in index
//                              order, AdamW in the epilogue on the elements the lane holds.  Workgroup (0,0) also adds
//                              the loss_b in a fixed order.
// The fp32-input MFMA is bit for bit a k-ordered fmaf chain, so nothing here depends on scheduling.
#include "mmr_common.h"
#include "scan_host.h"
#include "tip_mfma.h"

#include <math.h>

namespace mmr {

constexpr int TT_UU = 16;    // update kernel: MFMA steps (4 batch rows each) per trip of the K loop

// LDS: Fs[TT_BM][E + TT_PAD], Ls[TT_BM][64] (100 F Wc), Gt[64][TT_BM] (G, class-major)
static inline size_t tt_forward_lds(int E) { return ((size_t)TT_BM * (E + TT_PAD) + 2 * TT_BM * TT_CMAX) * sizeof(float); }

template <class T>
__global__ __launch_bounds__(256) void tip_train_forward_kernel(const T *__restrict__ f, const int64_t *__restrict__ y,
                                                                 const T *__restrict__ wct, const float *__restrict__ V,
                                                                 const float *__restrict__ W, int64_t B, int E, int C, int S,
                                                                 float alpha10, float beta, float *ws, float *__restrict__ loss_b,
                                                                 int32_t *__restrict__ pred, int32_t *__restrict__ status)
{
    extern __shared__ float4 tt_smem[];
    const int ldf = E + TT_PAD;
    float *Fs = reinterpret_cast<float *>(tt_smem);
    float *Ls = Fs + TT_BM * ldf;
    float *Gt = Ls + TT_BM * TT_CMAX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
    const int64_t b0 = (int64_t)blockIdx.x * TT_BM;

    // the feature block as fp32
    const int e4 = E / 4;
    for (int i = tid; i < TT_BM * e4; i += 256) {
        const int row = i / e4, c4 = i - row * e4;
        // rows past B repeat the last row: what is computed for them is never stored
        *reinterpret_cast<float4 *>(Fs + row * ldf + 4 * c4) = tt_load4<T>(f + (size_t)min(b0 + row, B - 1) * E + 4 * c4);
    }
    __syncthreads();

    // P = exp(beta*A - beta), parked in the workspace: wave w takes the chunks of 32 columns w, w+4, ...
    for (int s0 = wave * 32; s0 < S; s0 += 128) {
        f32x4 acc[2];
        tt_rows_times_block<float>(Fs, ldf, W, s0, S, E, acc[0], acc[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int s = s0 + 16 * j + r;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t b = b0 + 4 * h + reg;
                if (s < S && b < B) ws[(size_t)b * S + s] = expf(beta * acc[j][reg] - beta);
            }
        }
    }
    // the classifier columns, 100 F Wc: at most two chunks, given to the LAST waves -- the ones with the fewest chunks of S
    for (int c0 = (3 - wave) * 32; c0 < C; c0 += 128) {
        f32x4 acc[2];
        tt_rows_times_block<T>(Fs, ldf, wct, c0, C, E, acc[0], acc[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + 16 * j + r;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (c < C) Ls[(4 * h + reg) * TT_CMAX + c] = 100.f * acc[j][reg];
        }
    }
    __syncthreads();   // this workgroup's rows of P and Ls are complete

    // P V: wave w owns rows 4w..4w+3, lane c owns class c; s ascending, one fmaf chain per (row, class).  64 values of P
    // per row arrive in one coalesced load and are handed round from the lanes' registers
    float pv[4] = {0.f, 0.f, 0.f, 0.f};
    size_t prow[4];
    int64_t label[4];                        // fetched here, needed after the sum
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t b = min(b0 + 4 * wave + i, B - 1);
        prow[i] = (size_t)b * S;
        label[i] = y[b];
    }
    for (int sb = 0; sb < S; sb += 64) {
        float p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = ws[prow[i] + min(sb + lane, S - 1)] * tt_mask(sb + lane < S);
        }
        // always 64 steps, so that the loads of V are all in flight at once; past S the factor from P is zero and the fmaf
        // leaves pv as it is (lanes past C compute a duplicate of class C-1 that nobody reads)
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const float v = V[(size_t)min(sb + j, S - 1) * C + min(lane, C - 1)];
#pragma unroll
            for (int i = 0; i < 4; ++i) pv[i] = fmaf(tt_readlane(p[i], j), v, pv[i]);
        }
    }

    // softmax with the row maximum subtracted, loss_b, pred_b and the row of G
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 4 * wave + i;
        const int64_t b = b0 + row;
        const float L = lane < C ? Ls[row * TT_CMAX + lane] + alpha10 * pv[i] : -__builtin_inff();
        const float mx = wave_max(L);
        const float e = lane < C ? expf(L - mx) : 0.f;
        const float sum = wave_sum(e);
        const unsigned long long top = __ballot(lane < C && L == mx);
        const int64_t yb = label[i];
        const bool valid = yb >= 0 && yb < C;
        const float Ly = __shfl(L, valid ? (int)yb : 0, 64);
        // classes past C hold zeros: the dA stage below walks c in blocks of 8
        Gt[lane * TT_BM + row] = (valid && lane < C) ? (e / sum - (lane == (int)yb ? 1.f : 0.f)) / (float)B : 0.f;
        if (lane == 0 && b < B) {
            loss_b[b] = valid ? logf(sum) - (Ly - mx) : 0.f;
            if (pred) pred[b] = top ? __ffsll(top) - 1 : 0;
            if (!valid && status) atomicOr(status, 1);
        }
    }
    __syncthreads();

    // dA = beta * P * (10 alpha * G V^T), in place over this workgroup's rows of P: thread s, c ascending
    for (int s = tid; s < S; s += 256) {
        float acc[TT_BM];
#pragma unroll
        for (int i = 0; i < TT_BM; ++i) acc[i] = 0.f;
        float p[TT_BM];                      // this thread's column of P, fetched while the sum below runs
#pragma unroll
        for (int i = 0; i < TT_BM; ++i) p[i] = ws[(size_t)min(b0 + i, B - 1) * S + s];
        for (int c0 = 0; c0 < C; c0 += 8) {   // eight loads of V in flight; past C the factor from G is zero
            float v8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v8[u] = V[(size_t)s * C + min(c0 + u, C - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float v = v8[u];
#pragma unroll
                for (int q = 0; q < TT_BM / 4; ++q) {
                    const float4 g = *reinterpret_cast<const float4 *>(Gt + (c0 + u) * TT_BM + 4 * q);
                    acc[4 * q + 0] = fmaf(g.x, v, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(g.y, v, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(g.z, v, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(g.w, v, acc[4 * q + 3]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TT_BM; ++i) {
            const int64_t b = b0 + i;
            if (b < B) ws[(size_t)b * S + s] = beta * p[i] * (alpha10 * acc[i]);
        }
    }
}

// AdamW's per-step scalars, derived on the host in fp64
struct TipAdamW {
    double decay;       // 1 - lr * weight_decay
    double omb1;        // 1 - beta1
    double beta2;
    double omb2;        // 1 - beta2
    double step_size;   // lr / (1 - beta1^step)
    double bc2_sqrt;    // sqrt(1 - beta2^step)
    double eps;
};

// g = dA^T F for the tile s0..s0+15 x e0..e0+63 of [S,E]; K = B in index order (MFMA j sums b = 4j .. 4j+3 in that order).
// A[i][k] = dA[b][s0 + i] on lane (i = lane & 15, k = lane >> 4); B[k][j] = F[b][e0 + 4j + c] for accumulator c, so a lane
// ends with four consecutive e for each of its four rows s = s0 + 4*(lane >> 4) + reg.
template <class T>
__global__ __launch_bounds__(64) void tip_train_update_kernel(const float *__restrict__ dA, const T *__restrict__ f,
                                                               const float *__restrict__ loss_b, int64_t B, int E, int S,
                                                               float *__restrict__ W, float *__restrict__ m,
                                                               float *__restrict__ v, float *__restrict__ grad_out,
                                                               float *__restrict__ loss, TipAdamW a, int with_grad)
{
    const int lane = threadIdx.x, r = lane & 15, h = lane >> 4;
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        // lane l adds loss_b[l], loss_b[l + 64], ... in that order; the 64 partials meet in the xor butterfly
        float p = 0.f;
        for (int64_t b = lane; b < B; b += 64) p += loss_b[b];
        p = wave_sum(p);
        if (lane == 0) *loss = p / (float)B;
    }
    if (!with_grad) return;
    const int e0 = blockIdx.x * 64, s0 = blockIdx.y * 16;
    const float *ap = dA + min(s0 + r, S - 1);
    const T *bp = f + e0 + 4 * r;
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // TT_UU = 16 steps (64 rows of the batch) a trip, fetched during the trip before (one wave: nothing else hides the
    // latency).  A row past B is zero in the dA operand, and fmaf(0, x, acc) leaves acc as it is.
    float av[TT_UU], an[TT_UU];
    float4 bv[TT_UU], bn[TT_UU];
    auto fetch = [&](int64_t k0, float (&a_)[TT_UU], float4 (&b_)[TT_UU]) {
        if (k0 + 4 * TT_UU <= B) {   // a whole trip: one multiply for the trip, then the pointers step by four rows
            const float *pa = ap + (size_t)(k0 + h) * S;
            const T *pb = bp + (size_t)(k0 + h) * E;
#pragma unroll
            for (int u = 0; u < TT_UU; ++u) {
                a_[u] = *pa;
                b_[u] = tt_load4<T>(pb);
                pa += 4 * (size_t)S;
                pb += 4 * (size_t)E;
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < TT_UU; ++u) {
            const int64_t b = k0 + 4 * u + h;
            const size_t bc = (size_t)min(b, B - 1);
            a_[u] = ap[bc * S] * tt_mask(b < B);
            b_[u] = tt_load4<T>(bp + bc * E);
        }
    };
    fetch(0, av, bv);
    for (int64_t k0 = 0; k0 < B; k0 += 4 * TT_UU) {
        fetch(k0 + 4 * TT_UU, an, bn);
#pragma unroll
        for (int u = 0; u < TT_UU; ++u) {
            acc[0] = tt_mfma(av[u], bv[u].x, acc[0]);
            acc[1] = tt_mfma(av[u], bv[u].y, acc[1]);
            acc[2] = tt_mfma(av[u], bv[u].z, acc[2]);
            acc[3] = tt_mfma(av[u], bv[u].w, acc[3]);
        }
#pragma unroll
        for (int u = 0; u < TT_UU; ++u) {
            av[u] = an[u];
            bv[u] = bn[u];
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int s = s0 + 4 * h + reg;
        if (s >= S) continue;
        const size_t at = (size_t)s * E + e0 + 4 * r;
        const float g[4] = {acc[0][reg], acc[1][reg], acc[2][reg], acc[3][reg]};
        if (grad_out) *reinterpret_cast<float4 *>(grad_out + at) = make_float4(g[0], g[1], g[2], g[3]);
        if (!m) continue;
        const float4 w4 = *reinterpret_cast<const float4 *>(W + at), m4 = *reinterpret_cast<const float4 *>(m + at),
                     v4 = *reinterpret_cast<const float4 *>(v + at);
        float w_[4] = {w4.x, w4.y, w4.z, w4.w}, m_[4] = {m4.x, m4.y, m4.z, m4.w}, v_[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // torch's four lines, evaluated in fp64 from the fp32 state and the host's fp64 scalars, each stored value
            // rounded once.  (In fp32 the scalar 1 - beta2 alone is up to 0.8 ulp of v off, the two products before the
            // sum up to 1 ulp each: v could not be held within 2 ulp of the exact update.)  The W line reads the stored
            // m and v, as torch's does.
            const double gd = (double)g[c];
            m_[c] = (float)((double)m_[c] + (gd - (double)m_[c]) * a.omb1);
            v_[c] = (float)((double)v_[c] * a.beta2 + a.omb2 * gd * gd);
            const double denom = sqrt((double)v_[c]) / a.bc2_sqrt + a.eps;
            w_[c] = (float)((double)w_[c] * a.decay - a.step_size * (double)m_[c] / denom);
        }
        *reinterpret_cast<float4 *>(W + at) = make_float4(w_[0], w_[1], w_[2], w_[3]);
        *reinterpret_cast<float4 *>(m + at) = make_float4(m_[0], m_[1], m_[2], m_[3]);
        *reinterpret_cast<float4 *>(v + at) = make_float4(v_[0], v_[1], v_[2], v_[3]);
    }
}

template <class T>
static int tt_launch(const void *features, const int64_t *targets, int64_t B, int E, int C, int S, const void *wct,
                     const float *V, float *W, float *m, float *v, float alpha, float beta, const TipAdamW &a, float *loss,
                     int32_t *pred, float *grad_out, int32_t *status, float *ws, hipStream_t st)
{
    static DeviceOnce once;
    if (once.first())
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&tip_train_forward_kernel<T>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)tt_forward_lds(1024)));
    float *loss_b = ws + (size_t)B * S;
    hipLaunchKernelGGL(tip_train_forward_kernel<T>, dim3((unsigned)((B + TT_BM - 1) / TT_BM)), dim3(256), tt_forward_lds(E), st,
                       (const T *)features, targets, (const T *)wct, V, (const float *)W, B, E, C, S, 10.f * alpha, beta, ws,
                       loss_b, pred, status);
    MMR_CHECK_LAUNCH();
    const int with_grad = (m || grad_out) ? 1 : 0;
    const dim3 grid = with_grad ? dim3(E / 64, (S + 15) / 16) : dim3(1, 1);
    hipLaunchKernelGGL(tip_train_update_kernel<T>, grid, dim3(64), 0, st, (const float *)ws, (const T *)features,
                       (const float *)loss_b, B, E, S, W, m, v, grad_out, loss, a, with_grad);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_tip_adapter_f_workspace_bytes(int64_t B, int E, int C, int S)
{
    (void)E;
    (void)C;
    if (B <= 0 || S <= 0) return 0;
    return align_up(((size_t)B * (size_t)S + (size_t)B) * sizeof(float), 16);   // P / dA [B,S], then loss_b [B]
}

extern "C" int mmr_tip_adapter_f_step(const void *features, const int64_t *targets, mmr_dtype dtype, int64_t B, int E, int C,
                                      int S, const void *clip_weights_t, const float *cache_values, float *weight,
                                      float *exp_avg, float *exp_avg_sq, float alpha, float beta, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, int64_t step, float *loss, int32_t *pred,
                                      float *grad_out, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    const EntryCheck chk{"mmr_tip_adapter_f_step"};
    MMR_TRY(chk.dtype(dtype));
    MMR_CHECK_ARG(B >= 0 && C >= 1 && C <= TT_CMAX && S >= 1 && S <= 16384,
                  "mmr_tip_adapter_f_step: bad shape B=%lld C=%d S=%d (1 <= C <= 64, 1 <= S <= 16384)", (long long)B, C, S);
    MMR_CHECK_ARG(B <= (int64_t)0x7fffffff * TT_BM, "mmr_tip_adapter_f_step: B=%lld too large", (long long)B);
    MMR_TRY(dispatch_per(E, [](auto) -> int { return MMR_OK; }));
    MMR_CHECK_ARG((exp_avg == nullptr) == (exp_avg_sq == nullptr),
                  "mmr_tip_adapter_f_step: exp_avg and exp_avg_sq must both be given or both be NULL");
    if (exp_avg) {
        MMR_CHECK_ARG(step >= 1, "mmr_tip_adapter_f_step: step=%lld (counts from 1)", (long long)step);
        MMR_CHECK_ARG(isfinite(lr) && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && isfinite(eps) &&
                          isfinite(weight_decay),
                      "mmr_tip_adapter_f_step: bad optimizer scalars lr=%g beta1=%g beta2=%g eps=%g weight_decay=%g", lr, beta1,
                      beta2, eps, weight_decay);
    }
    if (B == 0) return MMR_OK;
    MMR_CHECK_ARG(features && targets && clip_weights_t && cache_values && weight && loss && workspace,
                  "mmr_tip_adapter_f_step: null pointer");
    MMR_TRY(chk.aligned16((uintptr_t)features | (uintptr_t)clip_weights_t | (uintptr_t)weight | (uintptr_t)exp_avg |
                              (uintptr_t)exp_avg_sq | (uintptr_t)grad_out | (uintptr_t)workspace,
                          "operands"));
    MMR_TRY(chk.workspace(workspace_bytes, mmr_tip_adapter_f_workspace_bytes(B, E, C, S)));
    TipAdamW a{};
    if (exp_avg) {
        a.decay = 1.0 - lr * weight_decay;
        a.omb1 = 1.0 - beta1;
        a.beta2 = beta2;
        a.omb2 = 1.0 - beta2;
        a.step_size = lr / (1.0 - pow(beta1, (double)step));
        a.bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
        a.eps = eps;
    }
    hipStream_t st = (hipStream_t)stream;
    return dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        return tt_launch<T>(features, targets, B, E, C, S, clip_weights_t, cache_values, weight, exp_avg, exp_avg_sq, alpha, beta,
                            a, loss, pred, grad_out, status, (float *)workspace, st);
    });
}
