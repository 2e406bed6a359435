// Perceptual hashes of decoded images for gfx950: imagehash's phash, dhash and whash (hash_size 8 or 16, every other
// argument at its default), from uint8 pixels to the uint64 [B, kinds, W] tensor the hash joins read (hash_join.hip).
//
// Replaces the per-file `imagehash.phash / dhash / whash` calls of the reference's clean-up tools
// (tool/find_repeated_in_same_folder.py:8-19).  All three start with Pillow's convert("L") and a LANCZOS resize, which is
// the 8-bit fixed-point separable convolution preprocess.hip already reproduces: the coefficient tables come from the host
// (preprocess.resample_tables(filter="lanczos")), the kernels only do int32 multiply-adds, so every intermediate byte
// equals Pillow's.  Three launches over a device array of per-image descriptors (mmr_image_hash_desc):
//   1. horizontal pass: each image row is read ONCE, turned into L in registers, staged in LDS, and resized to the
//      hs+1, 4*hs and S columns of the three hashes -> three uint8 planes [H][hs+1], [H][4hs], [H][S] in the workspace;
//   2. vertical pass: the small targets become [hs][hs+1] and [4hs][4hs] uint8; the S x S target is never stored, each
//      finished pixel goes into the integer sum of its (S/hs) x (S/hs) block (LDS partial sums, then 64-bit atomics);
//   3. finalize, one workgroup per image: dhash compares, phash's fp64 DCT sums against the host's cosine table, both
//      medians by rank counting, MSB-first packing and the status word.
// No launch depends on host knowledge of the image sizes: the grids are fixed and the workgroups stride over rows.
#include "mmr_common.h"

namespace mmr {

constexpr int IH_PRECISION_BITS = 32 - 8 - 2;        // Pillow Resample.c
constexpr int IH_ROUND = 1 << (IH_PRECISION_BITS - 1);
constexpr int IH_MAX_SIDE = MMR_IMAGE_HASH_MAX_SIDE;
constexpr int IH_LDS_BYTES = 32 * 1024;              // L rows of one workgroup; one row of the widest image fits twice
constexpr int IH_RB_MAX = 32;                        // input rows per workgroup step
constexpr int IH_THREADS = 256;
static_assert(IH_MAX_SIDE + 32 <= IH_LDS_BYTES, "one L row plus its slack must fit the LDS buffer");

typedef mmr_image_hash_desc IHDesc;

__host__ __device__ inline long long ih_a16(long long x) { return (x + 15) / 16 * 16; }

// S = max(2^floor(log2(min(W, H))), hs): imagehash's whash image_scale
__host__ __device__ inline int ih_side(int H, int W, int hs)
{
    const int m = H < W ? H : W;
    int s = 1;
    while (s * 2 <= m) s *= 2;
    return s > hs ? s : hs;
}

// one image's scratch inside the workspace, every part 16-byte aligned, absent kinds take no room
struct IHLayout { long long sums, small_d, small_p, plane_d, plane_p, plane_w, total; };
__host__ __device__ inline IHLayout ih_layout(int H, int W, int hs, int kinds)
{
    const long long S = ih_side(H, W, hs);
    IHLayout l;
    long long o = 0;
    l.sums = o;    o += (kinds & MMR_HASH_WHASH) ? ih_a16((long long)hs * hs * 8) : 0;
    l.small_d = o; o += (kinds & MMR_HASH_DHASH) ? ih_a16((long long)hs * (hs + 1)) : 0;
    l.small_p = o; o += (kinds & MMR_HASH_PHASH) ? ih_a16(16ll * hs * hs) : 0;
    l.plane_d = o; o += (kinds & MMR_HASH_DHASH) ? ih_a16((long long)H * (hs + 1)) : 0;
    l.plane_p = o; o += (kinds & MMR_HASH_PHASH) ? ih_a16((long long)H * 4 * hs) : 0;
    l.plane_w = o; o += (kinds & MMR_HASH_WHASH) ? ih_a16((long long)H * S) : 0;
    l.total = o;
    return l;
}

__host__ __device__ inline bool ih_table_ok(const int32_t *b, const int32_t *c, int k)
{
    return b && c && k >= 4 && (k & 3) == 0 && ((uintptr_t)c & 15) == 0 && ((uintptr_t)b & 7) == 0;
}

// everything a kernel relies on before it touches memory; the same test runs on the host copy of the descriptors in
// mmr_image_hashes_workspace_bytes.  An image that fails it is skipped by all three kernels and reported in its status.
__host__ __device__ inline bool ih_valid(const IHDesc &d, int hs, int kinds, size_t ws_bytes, bool check_ws)
{
    if (!d.img || d.H < 1 || d.W < 1 || d.H > IH_MAX_SIDE || d.W > IH_MAX_SIDE || (d.channels != 1 && d.channels != 3)) return false;
    if ((kinds & MMR_HASH_DHASH) && !(ih_table_ok(d.hb_d, d.hc_d, d.hk_d) && ih_table_ok(d.vb_d, d.vc_d, d.vk_d))) return false;
    if ((kinds & MMR_HASH_PHASH) && !(ih_table_ok(d.hb_p, d.hc_p, d.hk_p) && ih_table_ok(d.vb_p, d.vc_p, d.vk_p) && d.cos_table)) return false;
    if ((kinds & MMR_HASH_WHASH) && !(ih_table_ok(d.hb_w, d.hc_w, d.hk_w) && ih_table_ok(d.vb_w, d.vc_w, d.vk_w))) return false;
    if (check_ws) {
        const IHLayout l = ih_layout(d.H, d.W, hs, kinds);
        if (d.scratch_off < 0 || (d.scratch_off & 15) || (unsigned long long)d.scratch_off + (unsigned long long)l.total > ws_bytes) return false;
    }
    return true;
}

__device__ __forceinline__ int ih_clip8(int v)
{
    v >>= IH_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// byte * coefficient on the 24-bit multiplier (v_mad_i32_i24): |coefficient| < 2^23 is asserted where the tables are built
__device__ __forceinline__ int ih_bmul(uint32_t byte, int k) { return __mul24((int)byte, k); }
__device__ __forceinline__ int ih_dot4(uint32_t w, int k0, int k1, int k2, int k3)
{
    return ih_bmul(w & 0xffu, k0) + ih_bmul((w >> 8) & 0xffu, k1) + ih_bmul((w >> 16) & 0xffu, k2) + ih_bmul(w >> 24, k3);
}
__device__ __forceinline__ uint32_t ih_luma(uint32_t r, uint32_t g, uint32_t b)      // Pillow's L24 table form of convert("L")
{
    return (uint32_t)(__mul24((int)r, 19595) + __mul24((int)g, 38470) + __mul24((int)b, 7471) + 0x8000) >> 16;
}

// Lanes that share one output: a column (or pixel, in the vertical pass) with k taps is split over the smallest power of
// two of lanes that leaves each at most 16 taps, at most a wave.  9 columns of ~430 taps would otherwise keep 9 lanes busy.
__device__ __forceinline__ int ih_split(int k)
{
    const int need = (k + 15) >> 4;
    int g = 1;
    while (g < need && g < 64) g <<= 1;
    return g;
}

// the 4 bytes at byte offset `pos` of an LDS row (4-byte aligned base): two aligned dword reads and one v_alignbyte
__device__ __forceinline__ uint32_t ih_lds4(const uint8_t *row, int pos)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(row + (pos & ~3));
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(pos & 3));
}

// sum over each aligned group of G lanes (G a power of two <= 64), valid in the group's first lane at least: DPP within 16
// lanes (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: plain VALU), a cross-lane read for 32 and 64
__device__ __forceinline__ int ih_group_sum(int v, int G)
{
    if (G >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    if (G >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    if (G >= 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    if (G >= 16) v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
    if (G >= 32) v += __shfl_xor(v, 16, 64);
    if (G >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

// Horizontal pass of `nr` L rows held in LDS (row pitch `pitch`, at least 8 readable bytes behind each row) to one target:
// plane[row0 + r][x] for x < outW.  Taps go four at a time (coefficient rows are padded with zeros to whole groups of 4).
// G lanes of one wave share an output column, lane j takes the tap groups j, j + G, ...: neighbouring lanes read neighbouring
// LDS dwords and neighbouring int4 of the coefficient row.  Integer sums are exact in any order, so the bytes are Pillow's.
__device__ __forceinline__ void ih_h_target(const uint8_t *L, int pitch, int nr, int row0, const int32_t *hb, const int32_t *hc,
                                            int hk, int outW, uint8_t *__restrict__ plane)
{
    const int2 *bounds = reinterpret_cast<const int2 *>(hb);
    const int G = ih_split(hk);
    const int j = threadIdx.x & (G - 1);
    const int slots = ((hk >> 2) + G - 1) / G;              // tap groups per lane
    if (slots <= 4) {
        // the usual case (up to 1024 taps): a lane owns (column, j) for ALL rows of the step and keeps its coefficients in
        // registers, so the row loop is LDS reads and integer math only -- the tables are read once per step, not per row.
        // Every thread runs every round (the group sum is wave-wide); G divides 64 and the round size.
        const int total = outW * G;
        for (int base = 0; base < total; base += IH_THREADS) {
            const int it = base + threadIdx.x;
            const bool live = it < total;
            const int x = live ? it / G : 0;
            int4 k[4];
            int aoff[4];
            uint32_t sh = 0;
            {
                const int2 b = bounds[x];
                const int4 *k4 = reinterpret_cast<const int4 *>(hc + (size_t)x * hk);
                const int ng = live ? (b.y + 3) >> 2 : 0;
                sh = (uint32_t)(b.x & 3);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int g = j + i * G;
                    const bool on = i < slots && g < ng;    // a slot past the window multiplies the window's first bytes by 0
                    k[i] = on ? k4[g] : make_int4(0, 0, 0, 0);
                    aoff[i] = (b.x & ~3) + (on ? 4 * g : 0);
                }
            }
            for (int r = 0; r < nr; ++r) {
                const uint8_t *row = L + (size_t)r * pitch;
                int part = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < slots) {                        // uniform
                        const uint32_t *w = reinterpret_cast<const uint32_t *>(row + aoff[i]);
                        part += ih_dot4(__builtin_amdgcn_alignbyte(w[1], w[0], sh), k[i].x, k[i].y, k[i].z, k[i].w);
                    }
                }
                part = ih_group_sum(part, G);
                if (live && j == 0) plane[(size_t)(row0 + r) * outW + x] = (uint8_t)ih_clip8(part + IH_ROUND);
            }
        }
        return;
    }
    // more than 1024 taps per column (a side above ~1500 pixels to 9 columns): a wave per output, coefficients from memory
    const int total = nr * outW * G;
    for (int base = 0; base < total; base += IH_THREADS) {
        const int it = base + threadIdx.x;
        const bool live = it < total;
        int part = 0, r = 0, x = 0;
        if (live) {
            const int o = it / G;
            r = o / outW;
            x = o - r * outW;
            const int2 b = bounds[x];
            const int4 *k4 = reinterpret_cast<const int4 *>(hc + (size_t)x * hk);
            const uint8_t *row = L + (size_t)r * pitch;
            const int ng = (b.y + 3) >> 2;
            for (int g = j; g < ng; g += G) {
                const int4 k = k4[g];
                part += ih_dot4(ih_lds4(row, b.x + 4 * g), k.x, k.y, k.z, k.w);
            }
        }
        part = ih_group_sum(part, G);
        if (live && j == 0) plane[(size_t)(row0 + r) * outW + x] = (uint8_t)ih_clip8(part + IH_ROUND);
    }
}

__device__ __forceinline__ uint32_t ih_load4_unaligned(const uint8_t *p)
{
    typedef uint32_t u1 __attribute__((aligned(1)));
    return *reinterpret_cast<const u1 *>(p);
}

__global__ __launch_bounds__(IH_THREADS) void image_hash_h_kernel(const IHDesc *__restrict__ desc, int hs, int kinds,
                                                                  uint8_t *__restrict__ ws, size_t ws_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t L[IH_LDS_BYTES];
    const IHDesc d = desc[blockIdx.y];
    if (!ih_valid(d, hs, kinds, ws_bytes, true)) return;
    const IHLayout lay = ih_layout(d.H, d.W, hs, kinds);
    uint8_t *scratch = ws + d.scratch_off;
    if (blockIdx.x == 0 && (kinds & MMR_HASH_WHASH))        // the vertical pass adds into these; it runs after this kernel
        for (int i = threadIdx.x; i < hs * hs; i += IH_THREADS) reinterpret_cast<unsigned long long *>(scratch + lay.sums)[i] = 0ull;
    const int S = ih_side(d.H, d.W, hs);
    const int pitch = (d.W + 15) / 16 * 16 + 16;
    const int RB = min(IH_RB_MAX, IH_LDS_BYTES / pitch);    // >= 1: pitch <= IH_MAX_SIDE + 31
    const int qpr = (d.W + 3) >> 2;                         // groups of 4 pixels per row
    // a workgroup owns one contiguous share of the rows and walks it RB rows at a time
    const int share = (d.H + gridDim.x - 1) / gridDim.x;
    const int rend = min(d.H, ((int)blockIdx.x + 1) * share);
    for (int r0 = blockIdx.x * share; r0 < rend; r0 += RB) {
        const int nr = min(RB, rend - r0);
        __syncthreads();                                    // the previous step's readers are done with L
        // ---- stage: a thread turns 4 pixels (12 bytes of RGB, one dwordx3 load; consecutive lanes, consecutive bytes) into
        // one dword of L.  A row's last, partial group is read byte-wise: nothing is read past a row, hence past the image.
        for (int i = threadIdx.x; i < nr * qpr; i += IH_THREADS) {
            const int r = i / qpr, x0 = (i - r * qpr) * 4;
            uint32_t lw = 0;
            if (d.channels == 3) {
                const uint8_t *p = d.img + ((size_t)(r0 + r) * d.W + x0) * 3;
                if (x0 + 4 <= d.W) {
                    typedef uint32_t u3 __attribute__((ext_vector_type(3), aligned(1)));
                    const u3 v = *reinterpret_cast<const u3 *>(p);
                    lw = ih_luma(v.x & 0xffu, (v.x >> 8) & 0xffu, (v.x >> 16) & 0xffu)
                       | ih_luma(v.x >> 24, v.y & 0xffu, (v.y >> 8) & 0xffu) << 8
                       | ih_luma((v.y >> 16) & 0xffu, v.y >> 24, v.z & 0xffu) << 16
                       | ih_luma((v.z >> 8) & 0xffu, (v.z >> 16) & 0xffu, v.z >> 24) << 24;
                } else {
                    for (int c = 0; x0 + c < d.W; ++c) lw |= ih_luma(p[3 * c], p[3 * c + 1], p[3 * c + 2]) << (8 * c);
                }
            } else {
                const uint8_t *p = d.img + (size_t)(r0 + r) * d.W + x0;
                if (x0 + 4 <= d.W) lw = ih_load4_unaligned(p);
                else for (int c = 0; x0 + c < d.W; ++c) lw |= (uint32_t)p[c] << (8 * c);
            }
            *reinterpret_cast<uint32_t *>(L + (size_t)r * pitch + x0) = lw;
        }
        __syncthreads();
        if (kinds & MMR_HASH_DHASH) ih_h_target(L, pitch, nr, r0, d.hb_d, d.hc_d, d.hk_d, hs + 1, scratch + lay.plane_d);
        if (kinds & MMR_HASH_PHASH) ih_h_target(L, pitch, nr, r0, d.hb_p, d.hc_p, d.hk_p, 4 * hs, scratch + lay.plane_p);
        if (kinds & MMR_HASH_WHASH) ih_h_target(L, pitch, nr, r0, d.hb_w, d.hc_w, d.hk_w, S, scratch + lay.plane_w);
    }
}

// Vertical pass.  blockIdx.z picks the target: 0 dhash [hs][hs+1], 1 phash [4hs][4hs], 2 whash S x S (block sums only).
__global__ __launch_bounds__(IH_THREADS) void image_hash_v_kernel(const IHDesc *__restrict__ desc, int hs, int kinds,
                                                                  uint8_t *__restrict__ ws, size_t ws_bytes)
{
    __shared__ unsigned long long lsum[256];                // this workgroup's share of the hs x hs block sums
    const int z = blockIdx.z;
    const int kind = z == 0 ? MMR_HASH_DHASH : (z == 1 ? MMR_HASH_PHASH : MMR_HASH_WHASH);
    if (!(kinds & kind)) return;
    const IHDesc d = desc[blockIdx.y];
    if (!ih_valid(d, hs, kinds, ws_bytes, true)) return;
    const IHLayout lay = ih_layout(d.H, d.W, hs, kinds);
    uint8_t *scratch = ws + d.scratch_off;
    const bool isw = z == 2;
    const int S = ih_side(d.H, d.W, hs);
    const int outW = z == 0 ? hs + 1 : (z == 1 ? 4 * hs : S), outH = z == 0 ? hs : (z == 1 ? 4 * hs : S);
    const uint8_t *plane = scratch + (z == 0 ? lay.plane_d : (z == 1 ? lay.plane_p : lay.plane_w));
    const int2 *vb = reinterpret_cast<const int2 *>(z == 0 ? d.vb_d : (z == 1 ? d.vb_p : d.vb_w));
    const int32_t *vc = z == 0 ? d.vc_d : (z == 1 ? d.vc_p : d.vc_w);
    const int vk = z == 0 ? d.vk_d : (z == 1 ? d.vk_p : d.vk_w);
    uint8_t *out = z == 0 ? scratch + lay.small_d : (z == 1 ? scratch + lay.small_p : d.debug_w);     // nullable for z == 2
    const int cell = S / hs;                                // block side of whash, a power of two
    if (isw) {
        lsum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const int G = ih_split(vk);
    if (G == 1 && (outW & 3) == 0) {
        // a thread owns 4 neighbouring pixels of one output row: one dword load per tap, the coefficient shared
        const int quads = outW >> 2;
        const long long total = (long long)outH * quads;
        for (long long it = (long long)blockIdx.x * IH_THREADS + threadIdx.x; it < total; it += (long long)gridDim.x * IH_THREADS) {
            const int y = (int)(it / quads), x0 = (int)(it - (long long)y * quads) * 4;
            const int2 b = vb[y];
            const int32_t *k = vc + (size_t)y * vk;
            const uint8_t *p = plane + (size_t)b.x * outW + x0;
            int a0 = IH_ROUND, a1 = IH_ROUND, a2 = IH_ROUND, a3 = IH_ROUND;
            for (int t = 0; t < b.y; ++t) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(p + (size_t)t * outW);
                const int kk = k[t];
                a0 += ih_bmul(w & 0xffu, kk);
                a1 += ih_bmul((w >> 8) & 0xffu, kk);
                a2 += ih_bmul((w >> 16) & 0xffu, kk);
                a3 += ih_bmul(w >> 24, kk);
            }
            const int c[4] = {ih_clip8(a0), ih_clip8(a1), ih_clip8(a2), ih_clip8(a3)};
            if (out) {
                uint8_t *o = out + (size_t)y * outW + x0;   // debug_w is the caller's: no alignment assumed
                o[0] = (uint8_t)c[0]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[2]; o[3] = (uint8_t)c[3];
            }
            if (isw) {
                const int rowcell = (y / cell) * hs;
                if (cell >= 4) atomicAdd(&lsum[rowcell + x0 / cell], (unsigned long long)(c[0] + c[1] + c[2] + c[3]));
                else
                    for (int i = 0; i < 4; ++i) atomicAdd(&lsum[rowcell + (x0 + i) / cell], (unsigned long long)c[i]);
            }
        }
    } else {
        // G lanes of one wave share a pixel, lane j takes the taps j, j + G, ...: the small targets of a tall image have
        // hundreds to thousands of taps and a few hundred pixels
        const long long total = (long long)outH * outW * G, step = (long long)gridDim.x * IH_THREADS;
        const int j = threadIdx.x & (G - 1);
        for (long long base = (long long)blockIdx.x * IH_THREADS; base < total; base += step) {
            const long long it = base + threadIdx.x;
            const bool live = it < total;
            int part = 0, y = 0, x = 0;
            if (live) {
                const int o = (int)(it / G);
                y = o / outW;
                x = o - y * outW;
                const int2 b = vb[y];
                const int32_t *k = vc + (size_t)y * vk;
                const uint8_t *p = plane + (size_t)b.x * outW + x;
                for (int t = j; t < b.y; t += G) part += ih_bmul(p[(size_t)t * outW], k[t]);
            }
            for (int off = G >> 1; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
            if (live && j == 0) {
                const int c = ih_clip8(part + IH_ROUND);
                if (out) out[(size_t)y * outW + x] = (uint8_t)c;
                if (isw) atomicAdd(&lsum[(y / cell) * hs + x / cell], (unsigned long long)c);
            }
        }
    }
    if (isw) {
        __syncthreads();
        if ((int)threadIdx.x < hs * hs && lsum[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long *>(scratch + lay.sums) + threadIdx.x, lsum[threadIdx.x]);
    }
}

// 64 bits per wave, element 64w + lane -> bit 63 - lane of word w (numpy's bits.flatten(), most significant bit first)
__device__ __forceinline__ void ih_pack(bool bit, int ne, uint64_t *o)
{
    const unsigned long long m = __ballot(bit && (int)threadIdx.x < ne);
    if ((threadIdx.x & 63) == 0 && (int)threadIdx.x < ne) o[threadIdx.x >> 6] = __brevll(m);
}

// One workgroup per image.  hs * hs <= 256 hash elements, one per thread.
//
// phash, the only floating-point step.  With n = 4 hs, C[v][x] = cos(pi (2x+1) v / 2n) from the host's table, p the n x n bytes:
//     t[y][v] = sum_x p[y][x] * C[v][x]      (x ascending, every product and sum rounded to fp64: no fused multiply-add)
//     d[u][v] = 4 * sum_y C[u][y] * t[y][v]  (y ascending, likewise)
// so the host restatement (tests/image_hash_helpers.py) performs the same roundings and gets the same doubles.
// Error against the exact sum, u = 2^-53: a term of t is rounded once and carried through at most n - 1 additions, so
// |t~ - t| <= n u sum_x |p C| (1 + O(u)); a term of d carries that, its own product rounding and n - 1 additions:
// |d~ - d| <= 4 (2n + 1) u sum_y sum_x p |C||C| <= (2n + 1) u d[0][0], because |C| <= 1 and d[0][0] = 4 sum p (exact: C[0][x] = 1,
// integers below 2^53).  At n = 64 that is 129 * 1.11e-16 = 1.4e-14 d[0][0], against eps = 2^-32 d[0][0] = 2.3e-10 d[0][0]:
// four decades.  The median is the mean of two such values, same bound.  Hence a coefficient further than eps from the
// median has the sign of its exact difference whatever the summation order -- imagehash's scipy DCT included -- and
// status bit 0 marks the images where some coefficient is not.
__global__ __launch_bounds__(IH_THREADS) void image_hash_finalize_kernel(const IHDesc *__restrict__ desc, int hs, int kinds,
                                                                         uint8_t *__restrict__ ws, size_t ws_bytes,
                                                                         uint64_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ double t[64 * 16];
    __shared__ double dv[256];
    __shared__ double dmed[2];
    __shared__ unsigned long long sv[256], smed[2];
    __shared__ int flags;
    const int tid = threadIdx.x, ne = hs * hs, words = ne >> 6;
    const int nk = __popc(kinds & 7);
    uint64_t *o = out + (size_t)blockIdx.x * nk * words;
    const IHDesc d = desc[blockIdx.x];
    if (!ih_valid(d, hs, kinds, ws_bytes, true)) {          // uniform over the workgroup
        if (tid < nk * words) o[tid] = 0ull;
        if (tid == 0) status[blockIdx.x] = MMR_IMAGE_HASH_BAD_DESC;
        return;
    }
    const IHLayout lay = ih_layout(d.H, d.W, hs, kinds);
    const uint8_t *scratch = ws + d.scratch_off;
    if (tid == 0) flags = 0;
    __syncthreads();
    if (kinds & MMR_HASH_PHASH) {
        const int n = 4 * hs;
        const uint8_t *p = scratch + lay.small_p;
        const double *C = d.cos_table;
        for (int e = tid; e < n * hs; e += IH_THREADS) {
            const int y = e / hs, v = e - y * hs;
            double acc = 0.0;
            for (int x = 0; x < n; ++x) acc = __dadd_rn(acc, __dmul_rn((double)p[y * n + x], C[v * n + x]));
            t[e] = acc;
        }
        __syncthreads();
        if (tid < ne) {
            const int u = tid / hs, v = tid - u * hs;
            double acc = 0.0;
            for (int y = 0; y < n; ++y) acc = __dadd_rn(acc, __dmul_rn(C[u * n + y], t[y * hs + v]));
            dv[tid] = __dmul_rn(4.0, acc);
        }
        __syncthreads();
        bool bit = false;
        if (tid < ne) {                                     // the value at sorted position q lies in [less, leq)
            const double me = dv[tid];
            int less = 0, leq = 0;
            for (int i = 0; i < ne; ++i) { less += dv[i] < me; leq += dv[i] <= me; }
            if (less <= ne / 2 - 1 && ne / 2 - 1 < leq) dmed[0] = me;
            if (less <= ne / 2 && ne / 2 < leq) dmed[1] = me;
        }
        __syncthreads();
        if (tid < ne) {
            const double med = __dmul_rn(__dadd_rn(dmed[0], dmed[1]), 0.5);
            const double eps = __dmul_rn(0x1p-32, dv[0]);
            const double diff = __dsub_rn(dv[tid], med);
            bit = diff > eps;
            if (fabs(diff) <= eps) atomicOr(&flags, MMR_IMAGE_HASH_PHASH_NEAR_MEDIAN);
        }
        ih_pack(bit, ne, o);
        o += words;
    }
    if (kinds & MMR_HASH_DHASH) {
        const uint8_t *p = scratch + lay.small_d;
        bool bit = false;
        if (tid < ne) {
            const int r = tid / hs, c = tid - r * hs;
            bit = p[r * (hs + 1) + c + 1] > p[r * (hs + 1) + c];
        }
        ih_pack(bit, ne, o);
        o += words;
    }
    if (kinds & MMR_HASH_WHASH) {
        if (tid < ne) sv[tid] = reinterpret_cast<const unsigned long long *>(scratch + lay.sums)[tid];
        __syncthreads();
        if (tid < ne) {
            const unsigned long long me = sv[tid];
            int less = 0, leq = 0;
            for (int i = 0; i < ne; ++i) { less += sv[i] < me; leq += sv[i] <= me; }
            if (less <= ne / 2 - 1 && ne / 2 - 1 < leq) smed[0] = me;
            if (less <= ne / 2 && ne / 2 < leq) smed[1] = me;
        }
        __syncthreads();
        bool bit = false;
        if (tid < ne) bit = 2ull * sv[tid] > smed[0] + smed[1];
        if (tid == 0 && smed[0] == smed[1]) atomicOr(&flags, MMR_IMAGE_HASH_WHASH_TIED_MEDIAN);
        ih_pack(bit, ne, o);
    }
    __syncthreads();
    if (tid == 0) status[blockIdx.x] = flags;
}

}  // namespace mmr

using namespace mmr;

static bool ih_args_ok(const char *who, int hash_size, int kinds)
{
    if (hash_size != 8 && hash_size != 16) {
        set_error("%s: hash_size %d (8 or 16)", who, hash_size);
        return false;
    }
    if (kinds < 1 || kinds > 7) {
        set_error("%s: kinds mask %d (a non-empty subset of MMR_HASH_PHASH | MMR_HASH_DHASH | MMR_HASH_WHASH)", who, kinds);
        return false;
    }
    return true;
}

extern "C" size_t mmr_image_hash_scratch_bytes(int H, int W, int hash_size, int kinds)
{
    if (!ih_args_ok("mmr_image_hash_scratch_bytes", hash_size, kinds)) return 0;
    if (H < 1 || W < 1 || H > IH_MAX_SIDE || W > IH_MAX_SIDE) {
        set_error("mmr_image_hash_scratch_bytes: image %d x %d, sides must lie in [1, %d]", H, W, IH_MAX_SIDE);
        return 0;
    }
    return (size_t)ih_layout(H, W, hash_size, kinds).total;
}

extern "C" int mmr_image_hash_scratch_layout(int H, int W, int hash_size, int kinds, int64_t *offsets)
{
    MMR_CHECK_ARG(offsets, "mmr_image_hash_scratch_layout: null pointer");
    if (!mmr_image_hash_scratch_bytes(H, W, hash_size, kinds)) return MMR_EINVAL;
    const IHLayout l = ih_layout(H, W, hash_size, kinds);
    offsets[0] = l.sums; offsets[1] = l.small_d; offsets[2] = l.small_p;
    offsets[3] = l.plane_d; offsets[4] = l.plane_p; offsets[5] = l.plane_w;
    return MMR_OK;
}

extern "C" size_t mmr_image_hashes_workspace_bytes(const void *desc_host, int B, int hash_size, int kinds)
{
    if (!ih_args_ok("mmr_image_hashes_workspace_bytes", hash_size, kinds)) return 0;
    if (!desc_host || B < 1 || B > 65535) {
        set_error("mmr_image_hashes_workspace_bytes: %s", desc_host ? "B outside [1, 65535]" : "null descriptor array");
        return 0;
    }
    const IHDesc *d = (const IHDesc *)desc_host;
    unsigned long long need = 0;
    for (int i = 0; i < B; ++i) {
        if (d[i].H < 1 || d[i].W < 1 || d[i].H > IH_MAX_SIDE || d[i].W > IH_MAX_SIDE) {
            set_error("mmr_image_hashes_workspace_bytes: image %d is %d x %d, sides must lie in [1, %d]", i, d[i].H, d[i].W, IH_MAX_SIDE);
            return 0;
        }
        if (!ih_valid(d[i], hash_size, kinds, 0, false)) {
            set_error("mmr_image_hashes_workspace_bytes: descriptor %d: null pointer, channels not 1 or 3, or a coefficient table that is "
                      "not padded to groups of 4 taps and 16-byte aligned", i);
            return 0;
        }
        const unsigned long long total = (unsigned long long)ih_layout(d[i].H, d[i].W, hash_size, kinds).total;
        if (d[i].scratch_off < 0 || (d[i].scratch_off & 15)) {
            set_error("mmr_image_hashes_workspace_bytes: descriptor %d: scratch_off %lld must be a non-negative multiple of 16", i,
                      (long long)d[i].scratch_off);
            return 0;
        }
        if ((unsigned long long)d[i].scratch_off + total > need) need = (unsigned long long)d[i].scratch_off + total;
    }
    return (size_t)(need ? need : 16);
}

extern "C" int mmr_image_hashes(const void *desc_dev, int B, int hash_size, int kinds, uint64_t *out, int32_t *status,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ih_args_ok("mmr_image_hashes", hash_size, kinds)) return MMR_EINVAL;
    MMR_CHECK_ARG(desc_dev, "mmr_image_hashes: null descriptor array");
    MMR_CHECK_ARG(out && status && workspace, "mmr_image_hashes: null pointer");
    MMR_CHECK_ARG(B >= 0 && B <= 65535, "mmr_image_hashes: B=%d outside [0, 65535]", B);
    MMR_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)desc_dev & 7) == 0,
                  "mmr_image_hashes: workspace must be 16-byte aligned, out and the descriptors 8-byte aligned");
    MMR_CHECK_ARG(sizeof(IHDesc) == 168, "mmr_image_hashes: descriptor layout drifted");
    if (B == 0) return MMR_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const IHDesc *d = (const IHDesc *)desc_dev;
    uint8_t *ws = (uint8_t *)workspace;
    // fixed grids: the sizes live in device memory.  About 4096 workgroups per launch keep 256 CUs busy for any B; each
    // strides over its image's rows (pixels), and leaves at once when the image has fewer.
    const int hx = B >= 256 ? 16 : (B <= 8 ? 512 : 4096 / B);
    hipLaunchKernelGGL(image_hash_h_kernel, dim3(hx, B), dim3(IH_THREADS), 0, st, d, hash_size, kinds, ws, workspace_bytes);
    MMR_CHECK_LAUNCH();
    const int vx = B >= 256 ? 8 : (B <= 8 ? 256 : 2048 / B);
    hipLaunchKernelGGL(image_hash_v_kernel, dim3(vx, B, 3), dim3(IH_THREADS), 0, st, d, hash_size, kinds, ws, workspace_bytes);
    MMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(image_hash_finalize_kernel, dim3(B), dim3(IH_THREADS), 0, st, d, hash_size, kinds, ws, workspace_bytes, out, status);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
