// Greedy k-means++ seeding of a device-resident gallery for gfx950 (MI355X): sklearn's default start of the reference's
// KMeans(n_clusters=...) calls (code/search_image.py:185-292), exact and reproducible.  The definition is the comment
// above mmr_kmeanspp_seed in include/mmr.h; DESIGN.md section 3, "k-means++ seeding", has the measurements.
//
// One C call enqueues the whole seeding; nothing is read back and nothing on the host depends on the data:
//   kpp_prep_kernel     shift from the norm bound's sources; resets the call's state slot
//   kpp_init_kernel     step 0's weights (1 on live rows), their per-block sums, the live count and the lowest live row
//   per step c:
//   kpp_sample_kernel   one workgroup per trial: r = (variate * T) >> 53, then a two-level search -- the per-block sums
//                       find the block, the block's 256 weights find the row.  Every loop is bounded by the block count
//                       or by the block size.
//   kpp_dist_kernel     the gallery pass: 256 rows per workgroup, 16 lanes per row and four rows per wave pass
//                       (exact_dot.h's quarter-wave order), the <= 16 candidate rows staged in LDS as fp32.  A row is
//                       loaded and converted once and dotted with every candidate; lane t of the row's 16 lanes keeps
//                       trial t = min(closest, weight to candidate t), stores it and sums it over the block.
//   kpp_pick_kernel     adds the per-block sums of each trial, takes the smallest potential (ties to the lowest trial),
//                       writes indices[c], potentials[c] and the centre row, and leaves the winner's plane number in the
//                       state: the next step reads `closest` through it, nothing of size N is copied.
// The trial vectors live in two buffers of L planes [N] that alternate from step to step.  All sums of weights are int64,
// exact in any order; the only atomics are integer ones.  Vector stores and plain C++ only.
#include "mmr_common.h"
#include "exact_dot.h"
#include "range_common.h"
#include "scan_host.h"

#include <math.h>

#include <hip/hip_runtime.h>

namespace mmr {

constexpr int KPP_ROWS = MMR_KMEANSPP_BLOCK_ROWS;      // rows per workgroup of the pass = rows per block of the sampling
constexpr int KPP_LMAX = MMR_KMEANSPP_TRIALS_MAX;
constexpr long long KPP_WMAX = (1ll << 38) - 1;
constexpr int KPP_K_MAX = 65535;
constexpr int64_t KPP_N_MAX = (int64_t)1 << 24;
static_assert(KPP_ROWS == 256 && KPP_LMAX == 16, "the pass gives one of a row's 16 lanes to each trial, 16 rows per pass");

struct KppState {
    long long total;             // T: the sum of `closest`
    int32_t win;                 // the plane of the previous step's buffer that holds `closest`
    int32_t first_live;          // the lowest live row
    int32_t shift;
    int32_t pad;
    int32_t cand[KPP_LMAX];      // the rows the step's trials drew
};

__device__ __forceinline__ bool kpp_live(const uint32_t *row_mask, int64_t r)
{
    return !row_mask || ((row_mask[r >> 5] >> (r & 31)) & 1u);
}

__device__ __forceinline__ int32_t kpp_clamp_row(int32_t r, int64_t N)
{
    return r < 0 ? 0 : ((int64_t)r >= N ? (int32_t)(N - 1) : r);
}

// w = min(int64(trunc(max(d, 0) * 2^shift)), 2^38 - 1); 0 for a NaN d.  ldexp scales exactly.
__device__ __forceinline__ long long kpp_weight(double d, int shift)
{
    if (!(d == d)) return 0;
    const double x = ldexp(d > 0.0 ? d : 0.0, shift);
    return x >= 0x1p38 ? KPP_WMAX : (long long)x;
}

__global__ void kpp_prep_kernel(float host_bound, const float *__restrict__ dev_bound, int metric, KppState *__restrict__ s,
                                int32_t *__restrict__ shift_out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float G = host_bound > 0.f ? host_bound : 0.f;
    if (dev_bound) G = fmaxf(G, *dev_bound);
    const double g = (double)G;
    const double dmax = metric == 0 ? (4.0 * g) * g : 1.0 + g * g;
    const int shift = dmax == 0.0 ? 0 : 37 - ilogb(dmax);
    s->total = 0;
    s->win = 0;
    s->first_live = 0x7fffffff;
    s->shift = shift;
    s->pad = 0;
    for (int t = 0; t < KPP_LMAX; ++t) s->cand[t] = 0;
    *shift_out = shift;
}

// Inclusive prefix of an int64 over the wave
__device__ __forceinline__ long long kpp_wave_scan(long long v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long u = __shfl_up(v, off, 64);
        v += lane >= off ? u : 0;
    }
    return v;
}

// Exclusive and inclusive prefix of v over the 256 threads of the workgroup; every thread calls it.  sh: 4 words of LDS.
struct KppScan {
    long long excl, incl;
};
__device__ __forceinline__ KppScan kpp_block_scan(long long v, long long *sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long incl = kpp_wave_scan(v, lane);
    __syncthreads();                                   // the previous scan's readers are done with sh
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    long long base = 0;
    for (int w = 0; w < wave; ++w) base += sh[w];
    return {base + incl - v, base + incl};
}

// Step 0's weight vector: 1 on live rows, into plane 0 of a buffer, with its per-block sums; T = the live rows
__global__ __launch_bounds__(KPP_ROWS) void kpp_init_kernel(int64_t N, const uint32_t *__restrict__ row_mask,
                                                            long long *__restrict__ plane, long long *__restrict__ bsum,
                                                            KppState *__restrict__ s)
{
    __shared__ int cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * KPP_ROWS + tid;
    const bool live = row < N && kpp_live(row_mask, row);
    if (row < N) plane[row] = live ? 1 : 0;
    const unsigned long long b = __ballot(live);
    if (lane == 0) cnt[wave] = __popcll(b);
    if (b != 0 && lane == __ffsll((long long)b) - 1) atomicMin(&s->first_live, (int32_t)row);
    __syncthreads();
    if (tid == 0) {
        const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        bsum[blockIdx.x] = n;
        if (n > 0) atomicAdd((unsigned long long *)&s->total, (unsigned long long)n);
    }
}

// One workgroup per trial t: cand[t] = the smallest row whose inclusive prefix sum of `closest` exceeds
// r = (variate[t] * T) >> 53; the lowest live row when T == 0.  The id written is always a live row below N.
__global__ __launch_bounds__(KPP_ROWS) void kpp_sample_kernel(int64_t N, int nb, int planes, const long long *__restrict__ variates,
                                                              const long long *__restrict__ prev, const long long *__restrict__ prev_bsum,
                                                              const uint32_t *__restrict__ row_mask, KppState *__restrict__ s)
{
    __shared__ long long sh[4];
    __shared__ long long sh_r;
    __shared__ int sh_blk, sh_row;
    const int t = blockIdx.x, tid = threadIdx.x;
    int win = s->win;
    win = win < 0 ? 0 : (win >= planes ? planes - 1 : win);
    const long long T = s->total;
    const long long *w = prev + (size_t)win * (size_t)N, *bs = prev_bsum + (size_t)win * (size_t)nb;
    if (tid == 0) { sh_blk = -1; sh_row = -1; sh_r = 0; }
    __syncthreads();
    if (T > 0) {
        long long b = variates[t];
        b = b < 0 ? 0 : (b > (1ll << 53) - 1 ? (1ll << 53) - 1 : b);
        const unsigned long long hi = __umul64hi((unsigned long long)b, (unsigned long long)T);
        const unsigned long long lo = (unsigned long long)b * (unsigned long long)T;
        const long long r = (long long)((hi << 11) | (lo >> 53));
        // level 1: thread j owns the block sums [j0, j1)
        const int chunk = (nb + KPP_ROWS - 1) / KPP_ROWS;
        const int j0 = tid * chunk < nb ? tid * chunk : nb, j1 = j0 + chunk < nb ? j0 + chunk : nb;
        long long mine = 0;
        for (int j = j0; j < j1; ++j) mine += bs[j];
        const KppScan sc = kpp_block_scan(mine, sh);
        if (sc.excl <= r && r < sc.incl) {               // one thread at most: the weights are not negative
            long long acc = sc.excl;
            int blk = j0;
            for (int j = j0; j < j1; ++j) {
                const long long v = bs[j];
                blk = j;
                if (r < acc + v) break;
                acc += v;
            }
            sh_blk = blk;
            sh_r = r - acc;
        }
        __syncthreads();
        const int blk = sh_blk;
        if (blk >= 0) {
            // level 2: thread j owns row j of the block
            const long long r2 = sh_r;
            const int64_t row = (int64_t)blk * KPP_ROWS + tid;
            const long long v = row < N ? w[row] : 0;
            const KppScan sr = kpp_block_scan(v, sh);
            if (sr.excl <= r2 && r2 < sr.incl) sh_row = (int)row;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int32_t fl = kpp_clamp_row(s->first_live, N);
        int32_t id = sh_row;
        if (id < 0 || (int64_t)id >= N || !kpp_live(row_mask, id)) id = fl;
        s->cand[t] = id;
    }
}

// offset of element e of a staged candidate row: at PER = 8 four floats of padding after every eighth chunk keep the 16
// lanes' 16-byte reads (stride 32 bytes) on distinct banks
template <int PER>
__device__ __forceinline__ int kpp_lds_off(int e)
{
    return PER == 8 ? e + (e >> 6) * 4 : e;
}
template <int PER>
constexpr int kpp_lds_row() { return PER * 64 + (PER == 8 ? 32 : 0); }

template <typename T, int PER>
__device__ __forceinline__ void kpp_load_cand(const float *crow, int m, QuadQuery<T, PER> &q)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float *p = crow + kpp_lds_off<PER>((m + 16 * i) * PER);
        if constexpr (PER % 4 == 0) {
#pragma unroll
            for (int v = 0; v < PER / 4; ++v) {
                const float4 x = *reinterpret_cast<const float4 *>(p + v * 4);
                q.v[i][v * 4 + 0] = x.x; q.v[i][v * 4 + 1] = x.y; q.v[i][v * 4 + 2] = x.z; q.v[i][v * 4 + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int v = 0; v < PER / 2; ++v) {
                const float2 x = *reinterpret_cast<const float2 *>(p + v * 2);
                q.v[i][v * 2 + 0] = x.x; q.v[i][v * 2 + 1] = x.y;
            }
        }
    }
}

// The gallery pass of one step.  Workgroup b owns rows [256 b, 256 b + 256): 16 passes of 16 rows, one row per 16 lanes.
// FIRST (step 0): the squared norms are computed and stored, and the trial is the weight itself (no `closest` yet).
// dynamic LDS: L staged candidate rows of kpp_lds_row<PER>() floats.
template <typename T, int PER, bool FIRST>
__global__ __launch_bounds__(KPP_ROWS) void kpp_dist_kernel(const T *__restrict__ gal, int64_t N, int L, int metric, int nb, int planes,
                                                            const uint32_t *__restrict__ row_mask, double *__restrict__ norms,
                                                            const long long *__restrict__ prev, long long *__restrict__ out,
                                                            long long *__restrict__ bsum, const KppState *__restrict__ s)
{
    constexpr int E = PER * 64, LROW = kpp_lds_row<PER>();
    extern __shared__ float4 kpp_lds[];
    float *cl = reinterpret_cast<float *>(kpp_lds);
    __shared__ long long gsum[16][KPP_LMAX];
    __shared__ double cn[KPP_LMAX];
    const int tid = threadIdx.x, m = tid & 15, grp = tid >> 4;
    const int shift = s->shift;

    for (int v = tid; v < L * (E / 8); v += KPP_ROWS) {
        const int t = v / (E / 8), e0 = (v % (E / 8)) * 8;
        const int32_t c = kpp_clamp_row(s->cand[t], N);
        const uint4 x = *reinterpret_cast<const uint4 *>(gal + (size_t)c * E + e0);
        const uint32_t words[4] = {x.x, x.y, x.z, x.w};
        float *dst = cl + t * LROW;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            dst[kpp_lds_off<PER>(e0 + j)] = b16_to_f32<T>((uint16_t)(words[j >> 1] >> (16 * (j & 1))));
    }
    __syncthreads();
    if (grp < L) {                                      // n_c of candidate grp, in the order every n_i is taken in
        QuadQuery<T, PER> a;
        kpp_load_cand<T, PER>(cl + grp * LROW, m, a);
        const double n = quad_norm<T, PER>(a);
        if (m == 0) cn[grp] = n;
    }
    __syncthreads();

    int win = s->win;
    win = win < 0 ? 0 : (win >= planes ? planes - 1 : win);
    const long long *closest = FIRST ? nullptr : prev + (size_t)win * (size_t)N;
    long long acc = 0;
    for (int p = 0; p < 16; ++p) {
        const int64_t row = (int64_t)blockIdx.x * KPP_ROWS + p * 16 + grp;
        const bool valid = row < N;
        const int64_t lrow = valid ? row : N - 1;
        QuadRow<T, PER> gr;
        gr.load(gal + (size_t)lrow * E, m);
        double ni;
        if constexpr (FIRST) {
            ni = quad_norm<T, PER>(gr);
            if (valid && m == 0) norms[row] = ni;
        } else {
            ni = norms[lrow];
        }
        long long mine = 0;
        for (int t = 0; t < L; ++t) {
            QuadQuery<T, PER> cq;
            kpp_load_cand<T, PER>(cl + t * LROW, m, cq);
            const double dot = quad_dot<T, PER>(cq, gr);
            const double d = metric == 0 ? (ni + cn[t]) - 2.0 * dot : 1.0 - dot;
            if (m == t) mine = kpp_weight(d, shift);      // every lane of the row holds d; lane t alone needs trial t's weight
        }
        if (m < L) {
            if constexpr (!FIRST) {
                const long long c = closest[lrow];
                mine = c < mine ? c : mine;
            }
            if (!valid || !kpp_live(row_mask, lrow)) mine = 0;
            if (valid) out[(size_t)m * (size_t)N + (size_t)row] = mine;
            acc += mine;
        }
    }
    gsum[grp][m] = acc;
    __syncthreads();
    if (tid < L) {
        long long sum = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) sum += gsum[g][tid];
        bsum[(size_t)tid * (size_t)nb + blockIdx.x] = sum;
    }
}

// One workgroup: the L potentials, their arg-min (ties to the lowest trial), the step's outputs and the winner's plane
template <typename T>
__global__ __launch_bounds__(KPP_ROWS) void kpp_pick_kernel(const T *__restrict__ gal, int64_t N, int E, int L, int nb, int step,
                                                            const long long *__restrict__ bsum, KppState *__restrict__ s,
                                                            int32_t *__restrict__ indices, long long *__restrict__ potentials,
                                                            T *__restrict__ centers)
{
    __shared__ unsigned long long pot[KPP_LMAX];
    __shared__ int sh_row;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < KPP_LMAX) pot[tid] = 0;
    __syncthreads();
    for (int t = 0; t < L; ++t) {
        long long a = 0;
        for (int j = tid; j < nb; j += KPP_ROWS) a += bsum[(size_t)t * (size_t)nb + j];
        a = wave_sum(a);
        if (lane == 0) atomicAdd(&pot[t], (unsigned long long)a);
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int t = 1; t < L; ++t)
            if ((long long)pot[t] < (long long)pot[best]) best = t;
        const int32_t row = kpp_clamp_row(s->cand[best], N);
        s->win = best;
        s->total = (long long)pot[best];
        indices[step] = row;
        potentials[step] = (long long)pot[best];
        sh_row = row;
    }
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(gal + (size_t)sh_row * E);
    uint4 *dst = reinterpret_cast<uint4 *>(centers + (size_t)step * E);
    for (int v = tid; v < E / 8; v += KPP_ROWS) dst[v] = src[v];
}

struct KppPlan {
    int nb;
    size_t off_nb, off_state, off_norms, off_buf, buf_bytes, off_bsum, bsum_bytes, total;
};

static KppPlan make_kpp_plan(int64_t N, int L)
{
    KppPlan p{};
    p.nb = (int)((N + KPP_ROWS - 1) / KPP_ROWS);
    WsLayout l;
    p.off_nb = l.take(sizeof(float));
    p.off_state = l.take(sizeof(KppState));
    p.off_norms = l.take((size_t)N * 8);
    // two buffers of L planes, then two of their block sums: the second of each pair sits *_bytes behind the first
    p.off_buf = l.take((size_t)L * (size_t)N * 8);
    p.buf_bytes = l.take((size_t)L * (size_t)N * 8) - p.off_buf;
    p.off_bsum = l.take((size_t)L * (size_t)p.nb * 8);
    p.bsum_bytes = l.take((size_t)L * (size_t)p.nb * 8) - p.off_bsum;
    p.total = l.off;
    return p;
}
static_assert(sizeof(KppState) <= 256, "the state is one workspace slot");

static bool kpp_sizes_ok(int64_t N, int E, int K, int L)
{
    return N >= 1 && N <= KPP_N_MAX && scan_supports_E(E) && K >= 1 && K <= KPP_K_MAX && (int64_t)K <= N && L >= 1 && L <= KPP_LMAX;
}

template <typename T, int PER>
static int kpp_run(const T *gal, int64_t N, int K, int L, int metric, const uint32_t *row_mask, const long long *variates,
                   const NormBound &nb, int32_t *indices, long long *potentials, int32_t *shift, T *centers, char *ws,
                   const KppPlan &p, hipStream_t st)
{
    constexpr int E = PER * 64;
    KppState *s = (KppState *)(ws + p.off_state);
    double *norms = (double *)(ws + p.off_norms);
    long long *buf[2] = {(long long *)(ws + p.off_buf), (long long *)(ws + p.off_buf + p.buf_bytes)};
    long long *bsum[2] = {(long long *)(ws + p.off_bsum), (long long *)(ws + p.off_bsum + p.bsum_bytes)};
    const dim3 grid((unsigned)p.nb), block(KPP_ROWS);
    const size_t row_lds = (size_t)kpp_lds_row<PER>() * sizeof(float);

    hipLaunchKernelGGL(kpp_prep_kernel, dim3(1), dim3(64), 0, st, nb.host, nb.dev, metric, s, shift);
    MMR_CHECK_LAUNCH();
    // step 0 samples from the ones in plane 0 of buffer 1 and writes its single trial into plane 0 of buffer 0
    hipLaunchKernelGGL(kpp_init_kernel, grid, block, 0, st, N, row_mask, buf[1], bsum[1], s);
    MMR_CHECK_LAUNCH();
    for (int c = 0; c < K; ++c) {
        const int cur = c & 1, prv = cur ^ 1;
        const int Lc = c == 0 ? 1 : L, planes = c <= 1 ? 1 : L;      // planes the previous step wrote
        hipLaunchKernelGGL(kpp_sample_kernel, dim3(Lc), block, 0, st, N, p.nb, planes, variates + (size_t)c * L,
                           (const long long *)buf[prv], (const long long *)bsum[prv], row_mask, s);
        MMR_CHECK_LAUNCH();
        if (c == 0)
            hipLaunchKernelGGL((kpp_dist_kernel<T, PER, true>), grid, block, Lc * row_lds, st, gal, N, Lc, metric, p.nb, planes,
                               row_mask, norms, (const long long *)buf[prv], buf[cur], bsum[cur], (const KppState *)s);
        else
            hipLaunchKernelGGL((kpp_dist_kernel<T, PER, false>), grid, block, Lc * row_lds, st, gal, N, Lc, metric, p.nb, planes,
                               row_mask, norms, (const long long *)buf[prv], buf[cur], bsum[cur], (const KppState *)s);
        MMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(kpp_pick_kernel<T>, dim3(1), block, 0, st, gal, N, E, Lc, p.nb, c, (const long long *)bsum[cur], s,
                           indices, potentials, centers);
        MMR_CHECK_LAUNCH();
    }
    return MMR_OK;
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_kmeanspp_workspace_bytes(int64_t N, int E, int K, int L)
{
    if (!kpp_sizes_ok(N, E, K, L)) return 0;
    return make_kpp_plan(N, L).total;
}

extern "C" int mmr_kmeanspp_seed(const void *gallery, mmr_dtype dtype, int64_t N, int E, int K, int L, int metric,
                                 const uint32_t *row_mask, const int64_t *variates_dev, float gallery_norm_bound,
                                 const float *gallery_norm_bound_dev, int32_t *indices, int64_t *potentials, int32_t *shift,
                                 void *centers, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *fn = "mmr_kmeanspp_seed";
    const EntryCheck ck{fn};
    MMR_TRY(ck.dtype(dtype));
    if (dtype == MMR_F32) {
        set_error("%s: fp32 galleries are not supported (bf16 or fp16 only, the dtypes of mmr_cosine_assign)", fn);
        return MMR_ENOTSUP;
    }
    MMR_TRY(ck.scan_E(E));
    MMR_CHECK_ARG(N >= 1 && N <= KPP_N_MAX, "%s: N=%lld outside [1, 2^24]", fn, (long long)N);
    MMR_CHECK_ARG(K >= 1 && K <= KPP_K_MAX && (int64_t)K <= N, "%s: K=%d outside [1, min(65535, N)]", fn, K);
    MMR_CHECK_ARG(L >= 1 && L <= KPP_LMAX, "%s: L=%d outside [1, %d]", fn, L, KPP_LMAX);
    MMR_CHECK_ARG(metric == 0 || metric == 1, "%s: metric=%d (0 euclidean, 1 cosine)", fn, metric);
    MMR_TRY(ck.norm_bound(gallery_norm_bound));
    MMR_CHECK_ARG(gallery != nullptr && variates_dev != nullptr && centers != nullptr, "%s: null pointer (gallery / variates_dev / centers)", fn);
    MMR_CHECK_ARG(indices != nullptr && potentials != nullptr && shift != nullptr && workspace != nullptr,
                  "%s: null pointer (indices / potentials / shift / workspace)", fn);
    MMR_TRY(ck.aligned16((uintptr_t)gallery | (uintptr_t)centers, "gallery / centers"));
    MMR_CHECK_ARG((((uintptr_t)variates_dev | (uintptr_t)potentials) & 7) == 0, "%s: variates_dev / potentials must be 8-byte aligned", fn);
    MMR_CHECK_ARG((((uintptr_t)indices | (uintptr_t)shift) & 3) == 0, "%s: indices / shift must be 4-byte aligned", fn);
    MMR_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    MMR_TRY(ck.row_mask(row_mask));
    const KppPlan p = make_kpp_plan(N, L);
    MMR_TRY(ck.workspace(workspace_bytes, p.total));

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const NormBound nb = resolve_norm_bound(gallery, dtype, N, E, gallery_norm_bound, gallery_norm_bound_dev, (float *)(ws + p.off_nb), st);
    MMR_TRY(nb.rc);
    ProfScope prof(MMR_PROF_ROWWISE, st);
    return dispatch_elem(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        if constexpr (__is_same(T, float)) {
            return MMR_ENOTSUP;       // refused above
        } else {
            return dispatch_per(E, [&](auto per) -> int {
                constexpr int PER = decltype(per)::value;
                if constexpr (PER == 16) {
                    return MMR_ENOTSUP;   // E = 1024: refused by scan_E above
                } else {
                    return kpp_run<T, PER>((const T *)gallery, N, K, L, metric, row_mask, (const long long *)variates_dev, nb, indices,
                                           (long long *)potentials, shift, (T *)centers, ws, p, st);
                }
            });
        }
    });
}
