// Device stage of the JPEG encode (the host stage is jpeg_encode_host.cpp; the contract is in mmr.h, the arithmetic in
// DESIGN.md section "JPEG encode").  Two launches over a ragged batch, the mirror of jpeg.hip:
//   jpeg_planes_kernel   uint8 pixels -> uint8 component planes: RGBA over a background, libjpeg's rgb_ycc, box
//                        downsampling of the chroma (h2v1 / h2v2 with their alternating bias) and the edge expansion
//   jpeg_fdct_kernel     planes -> int16 coefficients: libjpeg's jfdctint (rows, then columns), division by the table,
//                        and the luma dummy blocks outside the image
// All integer work, so the coefficients are libjpeg-turbo's (Pillow's) and two runs give the same bytes.  The host knows
// every size, so both grids are exact: one lane per 4-sample run, one wave per 8 blocks, no stride loop.  The plane and
// coefficient layout is jpeg_geometry.h's; the owner search, the DCT constants and the transpose tile are jpeg_device.h's.
#include "mmr_common.h"

#include "jpeg_device.h"

namespace mmr {

constexpr int JENC_THREADS = 256;
constexpr int JENC_WAVES = JENC_THREADS / 64;

typedef mmr_jpeg_encode_desc EDesc;

// one pixel as R, G, B; four-channel input is composited over the background as Image.paste with the alpha mask does
__device__ __forceinline__ void jenc_pixel(const EDesc &d, int y, int x, int &R, int &G, int &Bl)
{
    const uint8_t *p = d.src + (long long)y * d.row_stride + (long long)x * d.channels;
    if (d.channels == 1) {
        R = G = Bl = p[0];
        return;
    }
    R = p[0]; G = p[1]; Bl = p[2];
    if (d.channels == 4) {
        const int a = p[3], na = 255 - a;
        int t = R * a + (d.background & 255) * na + 128;
        R = ((t >> 8) + t) >> 8;
        t = G * a + ((d.background >> 8) & 255) * na + 128;
        G = ((t >> 8) + t) >> 8;
        t = Bl * a + ((d.background >> 16) & 255) * na + 128;
        Bl = ((t >> 8) + t) >> 8;
    }
}

// component c (0 Y, 1 Cb, 2 Cr) of the pixel at (y, x), libjpeg's rgb_ycc_convert
__device__ __forceinline__ int jenc_sample(const EDesc &d, int c, int y, int x)
{
    int R, G, Bl;
    jenc_pixel(d, y, x, R, G, Bl);
    if (d.channels == 1) return R;
    if (c == 0) return (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16;
    if (c == 1) return (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16;
}

// A lane owns 4 consecutive samples of one plane row (the rows are multiples of 8 wide) and stores one dword.  Columns
// past the image repeat its last column; rows past it repeat the last DOWNSAMPLED row, whose own inputs repeat the last
// image row only up to a multiple of vmax -- libjpeg expands the input first, downsamples, then expands the result.
__global__ __launch_bounds__(JENC_THREADS) void jpeg_planes_kernel(const EDesc *__restrict__ desc, int B, uint8_t *__restrict__ ws,
                                                                   unsigned long long ws_bytes, long long total_runs)
{
    const long long u = (long long)blockIdx.x * JENC_THREADS + threadIdx.x;
    if (u >= total_runs) return;
    const EDesc d = desc[ragged_owner<true>(desc, B, u)];
    const long long nb = image_blocks(d), off = (u - d.run_first) * 4;
    if (off < 0 || off >= nb * 64 || d.plane_off < 0 || (unsigned long long)d.plane_off + (unsigned long long)nb * 64 > ws_bytes) return;
    const BlockAt at = locate(d, off, 64);
    const int c = at.c, hs = c == 0 ? 1 : d.hmax, vs = c == 0 ? 1 : d.vmax;       // the chroma planes are downsampled
    const int pitch = at.bw * 8;
    const int row = (int)(at.at / pitch), col = (int)(at.at % pitch);
    const int srow = min(row, (d.H + vs - 1) / vs - 1);       // the downsampled row this plane row repeats
    const int y0 = min(srow * vs, d.H - 1), y1 = min(srow * vs + vs - 1, d.H - 1);
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int oc = col + k;
        const int x0 = min(oc * hs, d.W - 1), x1 = min(oc * hs + hs - 1, d.W - 1);
        int v;
        if (hs == 1) {
            v = jenc_sample(d, c, y0, x0);
        } else if (vs == 1) {
            v = (jenc_sample(d, c, y0, x0) + jenc_sample(d, c, y0, x1) + (oc & 1)) >> 1;
        } else {
            v = (jenc_sample(d, c, y0, x0) + jenc_sample(d, c, y0, x1) + jenc_sample(d, c, y1, x0) + jenc_sample(d, c, y1, x1) + 1 + (oc & 1)) >> 2;
        }
        word |= (unsigned)v << (8 * k);
    }
    *(unsigned *)(ws + d.plane_off + off) = word;
}

// One 8-point pass of jfdctint (CONST_BITS 13, PASS1_BITS 2), in place.  FIRST: the row pass, which scales up by 4;
// otherwise the column pass, which takes that factor out again.
template <bool FIRST>
__device__ __forceinline__ void jenc_fdct8(int (&x)[8])
{
    constexpr int n = FIRST ? 11 : 15, r = 1 << (n - 1);
    const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
    const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        x[0] = (t10 + t11) * 4;
        x[4] = (t10 - t11) * 4;
    } else {
        x[0] = (t10 + t11 + 2) >> 2;
        x[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * F0_541;
    x[2] = (z1 + t13 * F0_765 + r) >> n;
    x[6] = (z1 - t12 * F1_847 + r) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1_175;
    const int a4 = t4 * F0_298, a5 = t5 * F2_053, a6 = t6 * F3_072, a7 = t7 * F1_501;
    z1 *= -F0_899; z2 *= -F2_562;
    z3 = z3 * (-F1_961) + z5;
    z4 = z4 * (-F0_390) + z5;
    x[7] = (a4 + z1 + z3 + r) >> n;
    x[5] = (a5 + z2 + z4 + r) >> n;
    x[3] = (a6 + z2 + z3 + r) >> n;
    x[1] = (a7 + z1 + z4 + r) >> n;
}

// libjpeg's quantisation: divide by 8 q (the DCT's scale and the table entry), round half away from zero
__device__ __forceinline__ int jenc_quant(int v, unsigned q)
{
    const unsigned dv = 8u * (q ? q : 1u), a = (unsigned)(v < 0 ? -v : v), m = (a + (dv >> 1)) / dv;
    return v < 0 ? -(int)m : (int)m;
}

// A wave takes 8 blocks; lane (block b = lane / 8, r = lane % 8) loads row r of its block as one 8-byte load, the 8 x 8
// transposes go through the wave's own padded LDS tile, and the lane stores coefficient row r as one 16-byte store (1 KiB
// per wave, contiguous).  A luma block outside the image (a dummy block) reads the block before it in its MCU's coding
// order that lies inside, and keeps only that block's DC.  Lanes past the last block neither load nor store; they still
// meet the barriers.
__global__ __launch_bounds__(JENC_THREADS) void jpeg_fdct_kernel(const EDesc *__restrict__ desc, int B, const uint8_t *__restrict__ qt,
                                                                 uint8_t *__restrict__ coef, const uint8_t *__restrict__ ws,
                                                                 unsigned long long ws_bytes, long long total_blocks)
{
    __shared__ int tile[JENC_WAVES][64 * TILE_STRIDE];
    const int lane = threadIdx.x & 63, r = lane & 7;
    int *t = tile[threadIdx.x >> 6];
    const long long g = (long long)blockIdx.x * (JENC_WAVES * 8) + (threadIdx.x >> 3);
    int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t *dst = nullptr;
    unsigned q[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    bool dummy = false;
    if (g < total_blocks) {
        const EDesc d = desc[ragged_owner<false>(desc, B, g)];
        const long long nb = image_blocks(d), ib = g - d.block_first;      // the block inside its image
        if (ib >= 0 && ib < nb && d.plane_off >= 0 && (unsigned long long)d.plane_off + (unsigned long long)nb * 64 <= ws_bytes) {
            const BlockAt at = locate(d, ib, 1);
            int by = (int)(at.at / at.bw), bx = (int)(at.at % at.bw);
            if (at.c == 0) {
                const int real_w = (d.W + 7) / 8, real_h = (d.H + 7) / 8;
                if (bx >= real_w || by >= real_h) {
                    dummy = true;
                    const int mx = bx / d.hmax, my = by / d.vmax;
                    int j = (by % d.vmax) * d.hmax + (bx % d.hmax) - 1;       // block 0 of an MCU is always inside
                    for (; j > 0; --j)
                        if (mx * d.hmax + j % d.hmax < real_w && my * d.vmax + j / d.hmax < real_h) break;
                    j = max(j, 0);
                    bx = mx * d.hmax + j % d.hmax;
                    by = my * d.vmax + j / d.hmax;
                }
            }
            const uint2 pv = *(const uint2 *)(ws + d.plane_off + at.plane + ((long long)by * 8 + r) * ((long long)at.bw * 8) + (long long)bx * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = (int)((pv.x >> (8 * k)) & 255u) - 128;
                x[4 + k] = (int)((pv.y >> (8 * k)) & 255u) - 128;
            }
            const int4 qv = *(const int4 *)(qt + d.qt_off + at.c * 128 + r * 16);
            const int qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[2 * k] = (unsigned)qw[k] & 0xffffu;
                q[2 * k + 1] = (unsigned)qw[k] >> 16;
            }
            dst = coef + d.coef_off + ib * 128 + r * 16;
        }
    }
    jenc_fdct8<true>(x);
    tile_put<false>(t, lane, x);
    __syncthreads();
    tile_get<true>(t, lane, x);         // column r of pass 1's result
    jenc_fdct8<false>(x);
    __syncthreads();
    tile_put<true>(t, lane, x);
    __syncthreads();
    tile_get<false>(t, lane, x);        // row r of the coefficients, natural order
    if (dst) {
        int o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (dummy && (r | k)) ? 0 : jenc_quant(x[k], q[k]);
        int4 v;
        v.x = (o[0] & 0xffff) | (int)((unsigned)o[1] << 16);
        v.y = (o[2] & 0xffff) | (int)((unsigned)o[3] << 16);
        v.z = (o[4] & 0xffff) | (int)((unsigned)o[5] << 16);
        v.w = (o[6] & 0xffff) | (int)((unsigned)o[7] << 16);
        *(int4 *)dst = v;
    }
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_jpeg_encode_workspace_bytes(const void *desc_host, int B)
{
    const BatchSize s = check_descriptors<EDesc>(
        "mmr_jpeg_encode_workspace_bytes", "encode", desc_host, B, false, [](const EDesc &e) { return image_blocks(e) * 16; },
        [](const EDesc &e, int i) {
            const bool channels = e.ncomp == 1 ? e.channels == 1 : (e.channels == 3 || e.channels == 4);
            if (!channels || !e.src || e.row_stride < (long long)e.W * e.channels || (e.background & ~0xffffff)) {
                set_error("mmr_jpeg_encode_workspace_bytes: descriptor %d: src is null, channels=%d does not go with %d components, row_stride=%lld "
                          "is less than a row, or background is no 24-bit colour", i, e.channels, e.ncomp, (long long)e.row_stride);
                return false;
            }
            if (!offsets_aligned(e)) set_error("mmr_jpeg_encode_workspace_bytes: descriptor %d: the offsets must be non-negative multiples of 16", i);
            return offsets_aligned(e);
        });
    if (!s.ok) return 0;
    if ((s.blocks + JENC_WAVES * 8 - 1) / (JENC_WAVES * 8) > 0x7fffffffll || (s.runs + JENC_THREADS - 1) / JENC_THREADS > 0x7fffffffll) {
        set_error("mmr_jpeg_encode_workspace_bytes: %lld blocks in one batch: its grids would pass 2^31 - 1 workgroups", s.blocks);
        return 0;
    }
    return (size_t)s.need;
}

extern "C" int mmr_jpeg_encode_device(const void *desc_dev, int B, const uint16_t *qt_dev, int16_t *coef_dev, void *ws, size_t ws_bytes,
                                      int64_t total_blocks, int64_t total_runs, void *stream)
{
    MMR_CHECK_ARG(B >= 0 && B <= 65535, "mmr_jpeg_encode_device: B=%d outside [0, 65535]", B);
    if (B == 0) return MMR_OK;
    MMR_CHECK_ARG(desc_dev && coef_dev && qt_dev && ws, "mmr_jpeg_encode_device: null pointer");
    MMR_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)qt_dev & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0,
                  "mmr_jpeg_encode_device: ws, coef_dev and qt_dev must be 16-byte aligned, the descriptors 8-byte aligned");
    MMR_CHECK_ARG(sizeof(EDesc) == 96, "mmr_jpeg_encode_device: descriptor layout drifted");
    MMR_CHECK_ARG(total_blocks >= 1 && total_runs == total_blocks * 16 && (unsigned long long)total_blocks * 64 <= ws_bytes,
                  "mmr_jpeg_encode_device: total_blocks=%lld, total_runs=%lld: expected at least one block, 16 runs per block and a workspace "
                  "of 64 bytes per block", (long long)total_blocks, (long long)total_runs);
    const long long g1 = (total_runs + JENC_THREADS - 1) / JENC_THREADS, g2 = (total_blocks + JENC_WAVES * 8 - 1) / (JENC_WAVES * 8);
    MMR_CHECK_ARG(g1 <= 0x7fffffffll && g2 <= 0x7fffffffll, "mmr_jpeg_encode_device: %lld blocks: the grids would pass 2^31 - 1 workgroups",
                  (long long)total_blocks);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    const EDesc *d = (const EDesc *)desc_dev;
    hipLaunchKernelGGL(jpeg_planes_kernel, dim3((unsigned)g1), dim3(JENC_THREADS), 0, st, d, B, (uint8_t *)ws, (unsigned long long)ws_bytes,
                       (long long)total_runs);
    MMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)g2), dim3(JENC_THREADS), 0, st, d, B, (const uint8_t *)qt_dev, (uint8_t *)coef_dev,
                       (const uint8_t *)ws, (unsigned long long)ws_bytes, (long long)total_blocks);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
