// The tile pipeline the MFMA gallery scans share: scan_kernel and scan16_kernel (topk_scan_body.h), scan_f32s_kernel and
// scan_split_kernel (search.hip), and the range, sweep, decide, assign and silhouette scans (*_scan_body.h).  The 16-bit
// ones are kernel templates over the element type, bf16_t or f16_t; the fp16 instantiations are compiled in translation
// units of their own (*_f16.hip).  Everything device-side here is force-inlined into the kernels.
//
// A scan workgroup owns the tiles [t0, t1) of the gallery.  It streams them through a ring of NBUF LDS slots filled by
// global_load_lds (3-deep by default: counted vmcnt, raw s_barrier), multiplies each tile with queries that stay resident
// in registers as MFMA B fragments, and keeps only what its epilogue needs: the per-(query, tile) maximum ("bucket max")
// and the per-(query, task) maximum for top-k, the candidate pairs for range search.
#pragma once
#include "mmr_common.h"

#include <type_traits>

namespace mmr {

// One gallery tile: ROWS rows of E elements of EB bytes, staged by WAVES waves.  A row is CH 16-byte chunks.
template <int E_, int EB, int ROWS_, int WAVES_>
struct TileGeom {
    static constexpr int E = E_, ROWS = ROWS_, WAVES = WAVES_;
    static constexpr int THREADS = WAVES * 64;
    static constexpr int CH = E * EB / 16;            // 16-byte chunks per row
    static constexpr int ROWB = E * EB;               // bytes per row
    static constexpr int TILE_BYTES = ROWS * ROWB;
    static constexpr int LOADS = ROWS * CH / 64;      // glds wave-instructions per tile
    static constexpr int LPW = LOADS / WAVES;         // per wave
    static_assert(LOADS % WAVES == 0, "tile loads must split evenly over the waves");
    static_assert(CH % 16 == 0, "XOR swizzle works on groups of 16 chunks");
};

// LDS position of chunk `chunk` of tile row `row`: XOR on the low 4 bits of the chunk index
__device__ __forceinline__ int swizzle(int chunk, int row) { return (chunk & ~15) | ((chunk ^ row) & 15); }

// Stage one tile into the LDS slot `slot`: the 16 B at slot offset 16p hold chunk swizzle(p % CH, row) of slot row
// row = p / CH.  The LDS image stays lane-linear for global_load_lds, while ds_read_b128 of 16 or 32 different rows at one
// chunk index is bank-conflict free.  Rows past N are clamped to row N - 1 and masked after the MFMA.
// NIMG = 2 (scan_split_kernel): the slot's G::ROWS rows are two images of one tile of G::ROWS / 2 rows, the hi image from
// src0 and the lo one from src1; the swizzle only sees the low 4 bits of the row, which both images share.
template <class G, int NIMG = 1, class T>
__device__ __forceinline__ void stage_tile(const T *src0, const T *src1, int64_t N, int tile, char *slot, int wave, int lane)
{
    constexpr int TR = G::ROWS / NIMG, EPC = 16 / sizeof(T);
    static_assert(TR % 16 == 0, "each image holds whole swizzle groups of rows");
#pragma unroll
    for (int i = 0; i < G::LPW; ++i) {
        const int instr = wave * G::LPW + i;
        const int p = instr * 64 + lane;
        const int row = p / G::CH;
        const int chunk = swizzle(p % G::CH, row);
        const int im = NIMG == 1 ? 0 : row / TR;      // wave-instruction uniform
        int64_t grow = (int64_t)tile * TR + (row - im * TR);
        grow = grow < N ? grow : N - 1;
        glds16((im ? src1 : src0) + grow * G::E + chunk * EPC, slot + instr * 1024);
    }
}

// The ring over the tiles [t0, t1): NBUF slots, PD = NBUF - 1 tiles staged ahead, LPW glds loads per wave and tile.
// Per tile t, in this order:
//   - wait until this wave's loads of tile t have landed (younger tiles may stay in flight) ...
//   - ... and after the raw barrier so have every other wave's; every wave is also done with tile t-1's slot;
//   - flush(): the previous tile's delayed bmax store, issued ahead of the staging;
//   - stage(t + PD, slot): overwrites tile t-1's slot;
//   - tile(t, slot): the multiply and the epilogue.
template <int NBUF, int LPW, class Stage, class Flush, class Tile>
__device__ __forceinline__ void tile_ring(int t0, int t1, Stage &&stage, Flush &&flush, Tile &&tile)
{
    static_assert(NBUF >= 2 && NBUF <= 4, "the wait counts below assume a prefetch distance of 1 to 3 tiles");
    constexpr int PD = NBUF - 1;
#pragma unroll
    for (int i = 0; i < PD; ++i)
        if (t0 + i < t1) stage(t0 + i, i);
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        const int younger = min(PD - 1, t1 - 1 - t);
        if (younger >= 2) wait_vmcnt<2 * LPW>();
        else if (younger == 1) wait_vmcnt<LPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        flush();
        int nxt = cur + PD; nxt = nxt >= NBUF ? nxt - NBUF : nxt;
        if (t + PD < t1) stage(t + PD, nxt);
        tile(t, cur);
        cur = cur + 1 >= NBUF ? 0 : cur + 1;
    }
}

// Counted LDS waits.  The A fragments run PF k-steps ahead of the MFMA that consumes them.  hipcc waits lgkmcnt(0) in
// front of every second MFMA when it schedules these reads itself (each wait then exposes the LDS latency and the MFMA
// pipe idles half the time), so the reads are issued as inline asm and retired with COUNTED waits: the fragment consumed
// at step s was issued PF steps earlier and n = min(PF - 1, steps left) younger reads may stay in flight (2n when every
// step reads two fragments).  The wait names its fragments "+v" so no use of them can be scheduled above it
// (cdna_hip_programming.md section 5.7, form ii).  n must be an immediate but is constant only after unrolling: the
// chain below folds to one s_waitcnt.
template <int M = 15>
__device__ __forceinline__ void wait_lgkmcnt(int n, bf16x8 &a)
{
    if (n == M) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(M));
    else if constexpr (M > 0) wait_lgkmcnt<M - 1>(n, a);
}
template <int M = 15>
__device__ __forceinline__ void wait_lgkmcnt(int n, bf16x8 &a, bf16x8 &b)
{
    if (n == M) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(M));
    else if constexpr (M > 0) wait_lgkmcnt<M - 1>(n, a, b);
}

__device__ __forceinline__ void ds_read_b128(bf16x8 &dst, const void *lds)
{
    asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"((uint32_t)(uintptr_t)lds));
}

// The two MFMA shapes of the scans by element type T: bf16_t or f16_t.  Fragments of both travel as bf16x8 (four VGPRs
// of raw bits: the LDS reads and the counted waits do not care); fp16 x fp16 products are exact in the fp32 accumulator
// like bf16's (11-bit significands, smallest product 2^-48).
template <class T>
__device__ __forceinline__ f32x16 mfma_32x32x16(const bf16x8 &a, const bf16x8 &b, const f32x16 &c)
{
    if constexpr (__is_same(T, f16_t))
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <class T>
__device__ __forceinline__ f32x4 mfma_16x16x32(const bf16x8 &a, const bf16x8 &b, const f32x4 &c)
{
    if constexpr (__is_same(T, f16_t))
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Resident queries of a 16-bit type T (bf16_t, f16_t): lane (c, h) of the wave holds, for k-step s, the 8 elements
// qp[s * STRIDE, +8), qp pointing at its query row plus its lane-group offset; zeros when it holds no live query.
template <int KSTEPS, int STRIDE, class T>
__device__ __forceinline__ void load_query_b16(const T *qp, bool live, bf16x8 (&bq)[KSTEPS])
{
    static_assert(sizeof(T) == 2, "16-bit elements");
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        bf16x8 v = *reinterpret_cast<const bf16x8 *>(qp + s * STRIDE);
        bq[s] = live ? v : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
}

// 8 fp32 -> hi and lo bf16 fragments (24 VALU instructions): hi = bf16(x), lo = bf16(x - hi)
__device__ __forceinline__ void split_bf16x8(const float4 &a0, const float4 &a1, bf16x8 &hi, bf16x8 &lo)
{
    const float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    union { bf16x8 v; uint32_t u[4]; } h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h.u[j] = pack_bf16x2(x[2 * j], x[2 * j + 1]);
        const float r0 = x[2 * j] - __uint_as_float(h.u[j] << 16);
        const float r1 = x[2 * j + 1] - __uint_as_float(h.u[j] & 0xffff0000u);
        l.u[j] = pack_bf16x2(r0, r1);
    }
    hi = h.v;
    lo = l.v;
}

// Resident queries, fp32 split into hi / lo bf16 fragments: k-step s holds the 8 elements qp[32s, +8)
template <int KSTEPS>
__device__ __forceinline__ void load_query_split(const float *qp, bool live, bf16x8 (&bqh)[KSTEPS], bf16x8 (&bql)[KSTEPS])
{
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        float4 a0 = *reinterpret_cast<const float4 *>(qp + s * 32), a1 = *reinterpret_cast<const float4 *>(qp + s * 32 + 4);
        if (!live) { a0 = make_float4(0.f, 0.f, 0.f, 0.f); a1 = a0; }
        split_bf16x8(a0, a1, bqh[s], bql[s]);
    }
}

// The 32x32x16 form (scan_kernel, range_scan_kernel): 32 resident queries per wave.  E <= 512 runs 8 waves (2 per SIMD,
// <= 256 VGPRs each); E = 768 needs 192 VGPRs for the resident queries alone, so it runs 4 waves at one wave per SIMD.
template <int E>
using Tile32 = TileGeom<E, 2, 32, E <= 512 ? 8 : 4>;
// CHAINS = 2 (one wave per SIMD): even and odd k-steps accumulate into separate registers, so a wave that has no SIMD
// partner to alternate with is not held to one dependent MFMA at a time
constexpr int chains_32x32(int waves) { return waves == 4 ? 2 : 1; }

// Dot products of one 32-row tile with the wave's 32 queries.  trow: the tile's LDS slot plus row c's offset.  Lane (c, h)
// holds in bq[s] the elements [16s + 8h, +8) of its query c and reads the same elements of tile row c.
// Result: acc[i] = dot(query c, tile row (i&3) + 8*(i>>2) + 4*h).  T: the operands' element type (mfma_32x32x16).
// SWAP (assign_scan_kernel, assign.hip): the two fragment layouts are the same, so passing (resident, tile) instead of
// (tile, resident) transposes the result: acc[i] = dot(resident row (i&3) + 8*(i>>2) + 4*h, tile row c) -- a lane then
// holds ONE gallery row against 16 of the wave's 32 resident rows, and a reduction over them is in-register.
template <int E, int CHAINS, int PF, class T = bf16_t, bool SWAP = false>
__device__ __forceinline__ f32x16 tile_dot_32x32(const char *trow, int c, int h, const bf16x8 (&bq)[E / 16])
{
    constexpr int KSTEPS = E / 16;
    f32x16 acc, acc2;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; }
    bf16x8 a[PF];
    auto issue = [&](int s, bf16x8 &dst) { ds_read_b128(dst, trow + swizzle(2 * s + h, c) * 16); };
#pragma unroll
    for (int s = 0; s < PF; ++s) issue(s, a[s]);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        wait_lgkmcnt((KSTEPS - 1 - s) < (PF - 1) ? (KSTEPS - 1 - s) : (PF - 1), a[s % PF]);
        const bool second = CHAINS == 2 && (s & 1);
        const bf16x8 &fa = SWAP ? bq[s] : a[s % PF], &fb = SWAP ? a[s % PF] : bq[s];
        if (second) acc2 = mfma_32x32x16<T>(fa, fb, acc2);
        else acc = mfma_32x32x16<T>(fa, fb, acc);
        if (s + PF < KSTEPS) {
            // the MFMA above must have READ a[s % PF] before the next load overwrites it: the empty statement ties the
            // accumulator to this point so the load cannot move above it
            if (second) asm volatile("" : "+v"(acc2)); else asm volatile("" : "+v"(acc));
            issue(s + PF, a[s % PF]);
        }
    }
    if (CHAINS == 2) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += acc2[i];
    }
    return acc;
}

// Split-bf16 dot products of one 16-row tile with the wave's 16 queries (scan_f32s_kernel, scan_split_kernel): the three
// products hi.hi, lo.hi and hi.lo on v_mfma_f32_16x16x32_bf16 in three accumulation chains, so no MFMA waits on the one
// issued just before it.  img_hi / img_lo: the tile's two bf16 images ([16 rows][E], swizzled).  Lane (r, g) reads row r,
// elements [32s + 8g, +8).  Both kernels take their bucket maxima from this one function, so they agree bit for bit.
// Result: acc[i] = dot(query r, tile row 4*g + i).
template <int E>
__device__ __forceinline__ f32x4 tile_dot_split3(const char *img_hi, const char *img_lo, int r, int g,
                                                 const bf16x8 (&bqh)[E / 32], const bf16x8 (&bql)[E / 32])
{
    constexpr int KSTEPS = E / 32;
    const int rowoff = r * (E * 2);
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f}, acc2 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc3 = (f32x4){0.f, 0.f, 0.f, 0.f};
    // hi / lo fragments run PF k-steps ahead of the MFMAs (deeper, 6, measured no faster)
    constexpr int PF = KSTEPS < 3 ? KSTEPS : 3;
    bf16x8 fh[PF], fl[PF];
    auto issue = [&](int s, bf16x8 &dh, bf16x8 &dl) {
        const int off = rowoff + (swizzle(4 * s + g, r) << 4);
        ds_read_b128(dh, img_hi + off);
        ds_read_b128(dl, img_lo + off);
    };
#pragma unroll
    for (int s = 0; s < PF && s < KSTEPS; ++s) issue(s, fh[s], fl[s]);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        bf16x8 &ah = fh[s % PF], &al = fl[s % PF];
        wait_lgkmcnt(2 * ((KSTEPS - 1 - s) < (PF - 1) ? (KSTEPS - 1 - s) : (PF - 1)), ah, al);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bqh[s], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bqh[s], acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bql[s], acc3, 0, 0, 0);
        if (s + PF < KSTEPS) {
            // the MFMAs above must have READ the fragments before the refill overwrites them
            asm volatile("" : "+v"(acc), "+v"(acc2), "+v"(acc3));
            issue(s + PF, ah, al);
        }
    }
    f32x4 d;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = acc[i] + (acc2[i] + acc3[i]);
    return d;
}

// Maximum over the live rows of a 16-row tile t, in every lane: acc[i] = dot(query, tile row 4*g + i).
// MASKED: `bits` holds the tile's 16 row-mask bits (row_mask_tile16); a row is live only if its bit is set.
template <bool MASKED = false>
__device__ __forceinline__ float tile_max_16(const f32x4 &acc, int t, int64_t N, int g, uint32_t bits = 0)
{
    float m = -INFINITY;
    const int64_t base = (int64_t)t * 16 + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, base + i < N && (!MASKED || ((bits >> (4 * g + i)) & 1u)) ? acc[i] : -INFINITY);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// Row masks (the *_masked entry points of include/mmr.h): bit r & 31 of word r >> 5 set = row r may be returned.  A
// workgroup owns at most 64 tiles, so at most 64 words (32-row tiles) or 33 (16-row tiles).  Lane l holds word w0 + l,
// loaded ONCE, before the ring: the ring's vmcnt waits and the k-loops' lgkmcnt waits are hand-counted, and a load
// inside the ring (vector or scalar) would break those counts.  The word is issued (mask_issue) in front of the
// resident-query loads and taken (mask_take) behind them: vector loads return in order, so the waits the query loads
// need anyway cover it, and the mask adds no wait of its own (tests/test_row_mask_isa.py checks the ISA).
// nw: the workgroup's words, all below ceil(N/32) because its tiles are; lanes >= nw hold 0.
struct MaskWord {
    uint32_t raw;
    bool ok;
};
__device__ __forceinline__ MaskWord mask_issue(const uint32_t *row_mask, int64_t w0, int nw, int lane)
{
    const bool ok = lane < nw;
    return {row_mask[ok ? w0 + lane : 0], ok};
}
__device__ __forceinline__ uint32_t mask_take(const MaskWord &m) { return m.ok ? m.raw : 0u; }

// The row-mask word of 32-row tile t from the lanes' words (load_mask_words with w0 = t0), bits at or past N cleared.
// The readlane takes a wave-uniform lane index: no memory access inside the ring.
__device__ __forceinline__ uint32_t row_mask_tile32(uint32_t words, int t, int t0, int64_t N)
{
    uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)words, t - t0);
    const int64_t left = N - (int64_t)t * 32;
    return left < 32 ? w & ((1u << (int)left) - 1u) : w;
}

// The 16 row-mask bits of 16-row tile t (load_mask_words with w0 = t0 >> 1), bits at or past N cleared.
__device__ __forceinline__ uint32_t row_mask_tile16(uint32_t words, int t, int t0, int64_t N)
{
    uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)words, (t >> 1) - (t0 >> 1));
    w = (w >> ((t & 1) * 16)) & 0xffffu;
    const int64_t left = N - (int64_t)t * 16;
    return left < 16 ? w & ((1u << (int)left) - 1u) : w;
}

// A row mask per query (the *_qmasked entry points): row q of row_masks is query q's mask in the format above, `shared`
// (nullable) one more mask AND-ed into every row.  The per-query scans (topk_scan_body.h, sweep_scan_body.h: QMASK)
// stage a task's words [tile][query] in LDS before the ring, for the reason given above.
struct QMaskArgs {
    const uint32_t *row_masks = nullptr;   // [Qc][stride] words of this pass's queries
    int64_t stride = 0;                    // words between two queries' rows, >= ceil(N/32)
    const uint32_t *shared = nullptr;      // [ceil(N/32)] AND-ed in; nullable
};

// Bucket maxima of one lane's query (top-k scans): bmax[tile * qpad + col] per tile, tmax[task * qpad + col] per task.
// A tile's maximum is stored one tile late, by flush() behind the next barrier, so the store does not sit between the
// loads the ring counts.  compute: the wave holds queries; writer: the lane that stores for its query.
struct BucketMax {
    float *bmax;
    int qpad, col;
    bool compute, writer;
    float task_max = -INFINITY, pend = -INFINITY;
    int pend_tile = -1;

    __device__ __forceinline__ void add(int t, float m) { task_max = fmaxf(task_max, m); pend = m; pend_tile = t; }
    __device__ __forceinline__ void flush() {
        if (compute && pend_tile >= 0 && writer) bmax[(size_t)pend_tile * qpad + col] = pend;
    }
    __device__ __forceinline__ void finish(float *tmax, int task) {
        if (compute && writer) {
            if (pend_tile >= 0) bmax[(size_t)pend_tile * qpad + col] = pend;
            tmax[(size_t)task * qpad + col] = task_max;
        }
    }
};

// ------------------------------------------------------------------ host side
// Tiles per scan task, at most: the task plan (scan_host.h: scan_tasks) and what the kernels size by it -- the candidate
// index of select_kernel (search.hip), the labels a sweep task stages (sweep_scan_body.h)
constexpr int SCAN_MAX_TPT = 64;
static inline bool scan_supports_E(int E) { return E == 128 || E == 256 || E == 512 || E == 768; }
// queries per scan pass: the bf16 / fp16 32x32 form's 8 x 32 (E <= 512) and scan16_kernel's 8 x 16 (E = 768); fp32
// galleries keep 16 queries per wave
static inline int scan_qmax(int E, mmr_dtype dt) { return (E <= 512 ? 256 : 128) / (dt == MMR_F32 ? 2 : 1); }

// f(std::integral_constant<int, E>{}) for a scan-supported E (scan_supports_E: anything else is 768)
template <class F>
static int scan_dispatch_E(int E, F &&f)
{
    switch (E) {
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        default: return f(std::integral_constant<int, 768>{});
    }
}

// Launch scan kernel K with `lds` bytes of dynamic LDS; the LDS limit is raised once per device and kernel, to lds_max:
// the most a call of K can ask for.  (The `once` is a static of this template: one per kernel and translation unit, so
// a kernel is launched from one translation unit only.)
template <auto K, class... A>
static int launch_scan_kernel_lds(unsigned grid, int threads, int lds, int lds_max, hipStream_t st, A... args)
{
    ProfScope prof(MMR_PROF_SCAN, st);
    static DeviceOnce once;
    if (once.first()) {
        MMR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), lds, st, args...);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
// ... for a kernel whose every call takes the same `lds` bytes
template <auto K, class... A>
static int launch_scan_kernel(unsigned grid, int threads, int lds, hipStream_t st, A... args)
{
    return launch_scan_kernel_lds<K>(grid, threads, lds, lds, st, args...);
}

}  // namespace mmr
