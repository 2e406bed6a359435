// A row mask per query for the deep top-k on gfx950 (MI355X): mmr_cosine_topk_deep_qmasked's kernels (its host side is
// deep_topk.hip's, shared with mmr_cosine_topk_deep) and mmr_row_masks_pack.
//   scan_qm_kernel / scan16_qm_kernel   the top-k scans scan_kernel / scan16_kernel (topk_scan_body.h, QMASK policy): the
//                                       task's mask words [tile][query] are staged in LDS behind the ring before the first
//                                       tile, and every lane tests its own query's word in the tile epilogue.
//   deep_rescore_qm_kernel              deep_rescore_kernel with the listed pair's query's mask row (deep_rescore_body.inc).
//   row_masks_pack_kernel               bool [Q,N] -> words [Q,stride], pad words zeroed, one launch.
// A translation unit of its own: the kernel sets of search.hip, search_f16.hip and deep_topk.hip are counted and compared
// by the ISA tests and tools/isa_diff.py, and stay as they are.
#include "mmr_common.h"
#include "exact_dot.h"
#include "scan_pipeline.h"
#include "topk_scan_body.h"
#include "topk_scan.h"
#include "scan_host.h"

#include <hip/hip_runtime.h>

namespace mmr {

constexpr int QMASK_LDS_MAX = 160 * 1024;          // gfx950: LDS per CU = the most one workgroup can take

template <class T, int E>
__global__ __launch_bounds__(ScanCfg<E>::THREADS, ScanCfg<E>::WAVES / 4) void scan_qm_kernel(
    const T *__restrict__ q, const T *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt, int qwaves, int qpad,
    float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_masks, int64_t stride,
    const uint32_t *__restrict__ shared)
{
    scan_body<T, E, false, true>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, nullptr, QMaskArgs{row_masks, stride, shared});
}

template <class T, int E>
__global__ __launch_bounds__(Scan16Cfg<E>::THREADS, 2) void scan16_qm_kernel(
    const T *__restrict__ q, const T *__restrict__ gal, int Q, int64_t N, int ntiles, int tpt, int qwaves, int qpad,
    float *__restrict__ bmax, float *__restrict__ tmax, const uint32_t *__restrict__ row_masks, int64_t stride,
    const uint32_t *__restrict__ shared)
{
    scan16_body<T, E, false, true>(q, gal, Q, N, ntiles, tpt, qwaves, qpad, bmax, tmax, nullptr, QMaskArgs{row_masks, stride, shared});
}

template <typename T, int PER>
__global__ __launch_bounds__(256) void deep_rescore_qm_kernel(const T *__restrict__ q, const T *__restrict__ gal, int64_t N,
                                                              int tile_rows, const uint32_t *__restrict__ row_mask,
                                                              const uint32_t *__restrict__ row_masks, int64_t stride,
                                                              unsigned long long *__restrict__ counter,
                                                              const uint64_t *__restrict__ tiles, int64_t tile_cap,
                                                              const double *__restrict__ thr_exact, uint64_t *__restrict__ surv_k,
                                                              uint64_t *__restrict__ surv_o, int64_t surv_cap)
{
    constexpr bool QM = true;
    const int64_t mask_stride = stride;
#include "deep_rescore_body.inc"
}

// One thread per (query, 32 rows): wave-wide ballots as in row_mask_pack_kernel, then the words [W, stride) of the query's
// row are zeroed by the threads of its last word's workgroup row.  grid (ceil(N / 256) or 1, Q).
__global__ __launch_bounds__(256) void row_masks_pack_kernel(const uint8_t *__restrict__ keep, const uint32_t *__restrict__ and_mask,
                                                             int64_t N, int64_t stride, uint32_t *__restrict__ out)
{
    const int64_t qi = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t W = (N + 31) >> 5;
    const uint64_t bits = __ballot(r < N && keep[qi * N + (r < N ? r : 0)] != 0);
    const int64_t w = r >> 5;
    uint32_t *o = out + qi * stride;
    if ((lane & 31) == 0 && w < W) {
        uint32_t v = (uint32_t)(bits >> (lane & 32));
        if (and_mask) v &= and_mask[w];
        o[w] = v;
    }
    if (blockIdx.x == 0)
        for (int64_t p = W + threadIdx.x; p < stride; p += 256) o[p] = 0u;
}

static int ring_bytes(int E)
{
    return scan_dispatch_E(E, [&](auto e) {
        constexpr int EE = decltype(e)::value;
        if constexpr (EE == 768) return (int)Scan16Cfg<EE>::LDS;
        else return (int)ScanCfg<EE>::LDS;
    });
}

int qmask_scan_tpt(int E, int qc, int tpt)
{
    const int cap = (QMASK_LDS_MAX - ring_bytes(E)) / qmask_lds_bytes(1, qc);
    return tpt < cap ? tpt : cap;
}

int launch_topk_scan_qmasked(mmr_dtype scan_dtype, int E, const void *q, const void *gal, int Qc, int64_t N, int ntiles, int tpt,
                             int qpad, float *bmax, float *tmax, const uint32_t *row_masks, int64_t stride,
                             const uint32_t *shared, hipStream_t st)
{
    const int lds = ring_bytes(E) + qmask_lds_bytes(tpt, qpad);
    if (scan_dtype == MMR_F32 || tpt < 1 || tpt > SCAN_MAX_TPT || lds > QMASK_LDS_MAX) {
        set_error("per-query scan: plan E=%d tpt=%d qpad=%d (%d bytes of LDS) unsupported", E, tpt, qpad, lds);
        return MMR_EIO;
    }
    const unsigned ntasks = (unsigned)((ntiles + tpt - 1) / tpt);
    return scan_dispatch_E(E, [&](auto e) {
        return dispatch_elem(scan_dtype, [&](auto tag) -> int {
            constexpr int EE = decltype(e)::value;
            using T = typename decltype(tag)::type;
            if constexpr (__is_same(T, float)) return MMR_EIO;
            else if constexpr (EE == 768)
                return launch_scan_kernel_lds<&scan16_qm_kernel<T, EE>>(ntasks, Scan16Cfg<EE>::THREADS, lds, QMASK_LDS_MAX, st,
                                                                        (const T *)q, (const T *)gal, Qc, N, ntiles, tpt, qpad / 16, qpad,
                                                                        bmax, tmax, row_masks, stride, shared);
            else
                return launch_scan_kernel_lds<&scan_qm_kernel<T, EE>>(ntasks, ScanCfg<EE>::THREADS, lds, QMASK_LDS_MAX, st, (const T *)q,
                                                                      (const T *)gal, Qc, N, ntiles, tpt, qpad / 32, qpad, bmax, tmax,
                                                                      row_masks, stride, shared);
        });
    });
}

int launch_deep_rescore_qmasked(mmr_dtype dtype, int E, const void *q, const void *gal, int64_t N, int tile_rows,
                                const uint32_t *row_mask, const uint32_t *row_masks, int64_t stride, unsigned long long *counter,
                                const uint64_t *tiles, int64_t tile_cap, const double *thr_exact, uint64_t *surv_k,
                                uint64_t *surv_o, int64_t surv_cap, hipStream_t st)
{
    const dim3 grid(grid_1d(tile_cap, 4, 8192));
    scan_dispatch_E(E, [&](auto e) {
        return dispatch_elem(dtype, [&](auto tag) -> int {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL((deep_rescore_qm_kernel<T, decltype(e)::value / 64>), grid, dim3(256), 0, st, (const T *)q,
                               (const T *)gal, N, tile_rows, row_mask, row_masks, stride, counter, tiles, tile_cap, thr_exact, surv_k,
                               surv_o, surv_cap);
            return MMR_OK;
        });
    });
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" int mmr_row_masks_pack(const uint8_t *keep, const uint32_t *and_mask, int Q, int64_t N, int64_t stride, uint32_t *out,
                                  void *stream)
{
    const char *fn = "mmr_row_masks_pack";
    MMR_CHECK_ARG(N >= 0 && N < 0x7fffffff, "%s: N=%lld outside [0, 2^31-1)", fn, (long long)N);
    MMR_CHECK_ARG(Q >= 0 && Q <= 65535, "%s: Q=%d outside [0, 65535]", fn, Q);
    MMR_CHECK_ARG(stride >= (N + 31) / 32, "%s: stride=%lld below ceil(N/32)=%lld words", fn, (long long)stride,
                  (long long)((N + 31) / 32));
    if (Q == 0 || stride == 0) return MMR_OK;
    MMR_CHECK_ARG(out && (keep || N == 0), "%s: null pointer", fn);
    MMR_CHECK_ARG((((uintptr_t)out | (uintptr_t)and_mask) & 3) == 0, "%s: out / and_mask must be 4-byte aligned", fn);
    const int64_t bx = (N + 255) / 256;
    hipLaunchKernelGGL(row_masks_pack_kernel, dim3((unsigned)(bx > 0 ? bx : 1), (unsigned)Q), dim3(256), 0, (hipStream_t)stream, keep,
                       and_mask, N, stride, out);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
