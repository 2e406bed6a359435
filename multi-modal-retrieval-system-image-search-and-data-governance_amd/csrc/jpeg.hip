// Device stage of the JPEG decode (the host stage is jpeg_host.cpp; the contract is in mmr.h, the arithmetic in DESIGN.md
// section "JPEG decode").  Two launches over a ragged batch whose sizes live in device memory:
//   jpeg_idct_kernel    int16 coefficients -> uint8 component planes: dequantise, libjpeg's jidctint (columns, then rows)
//   jpeg_color_kernel   planes -> uint8 [H, W, 3]: libjpeg's fancy h2v1 / h2v2 upsampling and YCbCr -> RGB
// All integer work, so the bytes are libjpeg-turbo's (Pillow's) and two runs give the same bytes.  The plane and coefficient
// layout is jpeg_geometry.h's; the owner search, the DCT constants and the transpose tile are jpeg_device.h's.
#include "mmr_common.h"

#include "jpeg_device.h"

namespace mmr {

constexpr int JP_THREADS = 256;
constexpr int JP_WAVES = JP_THREADS / 64;
constexpr int JP_MAX_GRID = 2048;

typedef mmr_jpeg_desc JDesc;

// a row without components (a file the host stage did not decode) has neither blocks nor runs, whatever else it holds
__host__ __device__ __forceinline__ long long jp_blocks(const JDesc &d) { return d.ncomp == 0 ? 0 : image_blocks(d); }
__host__ __device__ __forceinline__ long long jp_runs(const JDesc &d) { return d.ncomp == 0 ? 0 : ((long long)d.H * d.W + 3) / 4; }

// the unit list cut into gridDim.x contiguous spans, each a multiple of `step` units
__device__ __forceinline__ long long jp_span(long long total, int step)
{
    const long long per = (total + gridDim.x - 1) / gridDim.x;
    return (per + step - 1) / step * step;
}

// One 8-point pass of jidctint (CONST_BITS 13), in place; `s` is the descale shift of the pass.
__device__ __forceinline__ void jp_idct8(int (&x)[8], const int s)
{
    int z1 = (x[2] + x[6]) * F0_541;
    const int t2 = z1 - x[6] * F1_847, t3 = z1 + x[2] * F0_765;
    const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * F1_175;
    a0 *= F0_298; a1 *= F2_053; a2 *= F3_072; a3 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562;
    z3 = z3 * (-F1_961) + z5;
    z4 = z4 * (-F0_390) + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const int r = 1 << (s - 1);
    x[0] = (t10 + a3 + r) >> s; x[7] = (t10 - a3 + r) >> s;
    x[1] = (t11 + a2 + r) >> s; x[6] = (t11 - a2 + r) >> s;
    x[2] = (t12 + a1 + r) >> s; x[5] = (t12 - a1 + r) >> s;
    x[3] = (t13 + a0 + r) >> s; x[4] = (t13 - a0 + r) >> s;
}

__device__ __forceinline__ int jp_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// A wave takes 8 blocks; lane (block b = lane / 8, r = lane % 8) loads coefficient row r of its block as one 16-byte load
// (1 KiB per wave, contiguous: the batch's blocks are laid end to end), the 8 x 8 transposes go through the wave's own
// padded LDS tile.  Lanes past the last block neither load nor store; they still meet the barriers.
__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const JDesc *__restrict__ desc, int B,
                                                               const uint8_t *__restrict__ coef, const uint8_t *__restrict__ qt,
                                                               uint8_t *__restrict__ ws, unsigned long long ws_bytes)
{
    __shared__ int tile[JP_WAVES][64 * TILE_STRIDE];
    const int lane = threadIdx.x & 63, r = lane & 7;
    int *t = tile[threadIdx.x >> 6];
    const long long total = desc[B - 1].block_first + jp_blocks(desc[B - 1]);
    // a workgroup takes one contiguous span of the block list, so that a lane's next block mostly has the owner of its last
    // one and the search is skipped; the bounds depend on blockIdx alone, so every lane meets every barrier
    const long long span = jp_span(total, JP_WAVES * 8), begin = (long long)blockIdx.x * span, end = min(total, begin + span);
    JDesc d = {};
    long long nb = 0;
    for (long long base = begin; base < end; base += JP_WAVES * 8) {
        const long long g = base + (threadIdx.x >> 3);
        int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint8_t *dst = nullptr;
        if (g < end) {
            if (g < d.block_first || g - d.block_first >= nb) {
                d = desc[ragged_owner<false>(desc, B, g)];
                nb = jp_blocks(d);
            }
            const long long lb = g - d.block_first;            // the block inside its image
            if (lb >= 0 && lb < nb && d.plane_off >= 0 && (unsigned long long)d.plane_off + (unsigned long long)nb * 64 <= ws_bytes) {
                const int4 cv = *(const int4 *)(coef + d.coef_off + lb * 128 + r * 16);
                const BlockAt at = locate(d, lb, 1);
                const int4 qv = *(const int4 *)(qt + d.qt_off + at.c * 128 + r * 16);
                const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[2 * k] = (int)(short)(cw[k] & 0xffff) * (int)(qw[k] & 0xffff);
                    x[2 * k + 1] = (cw[k] >> 16) * (int)((unsigned)qw[k] >> 16);
                }
                const long long by = at.at / at.bw, bx = at.at % at.bw;
                dst = ws + d.plane_off + at.plane + (by * 8 + r) * ((long long)at.bw * 8) + bx * 8;
            }
        }
        tile_put<false>(t, lane, x);
        __syncthreads();
        tile_get<true>(t, lane, x);         // column r of the block
        jp_idct8(x, 11);
        __syncthreads();
        tile_put<true>(t, lane, x);
        __syncthreads();
        tile_get<false>(t, lane, x);        // row r of pass 1's result
        jp_idct8(x, 18);
        if (dst) {
            uint2 o;
            o.x = (unsigned)jp_clamp255(x[0] + 128) | ((unsigned)jp_clamp255(x[1] + 128) << 8) | ((unsigned)jp_clamp255(x[2] + 128) << 16) |
                  ((unsigned)jp_clamp255(x[3] + 128) << 24);
            o.y = (unsigned)jp_clamp255(x[4] + 128) | ((unsigned)jp_clamp255(x[5] + 128) << 8) | ((unsigned)jp_clamp255(x[6] + 128) << 16) |
                  ((unsigned)jp_clamp255(x[7] + 128) << 24);
            *(uint2 *)dst = o;
        }
        __syncthreads();
    }
}

// one upsampled chroma sample at output pixel (y, x); the plane's real size is dh x dw, its edges replicate
__device__ __forceinline__ int jp_chroma(const uint8_t *__restrict__ p, int pitch, int dw, int dh, int hs, int vs, int y, int x)
{
    if (hs == 1) return p[(long long)y * pitch + x];
    const int i = x >> 1, odd = x & 1;
    const int in = odd ? min(i + 1, dw - 1) : max(i - 1, 0);
    if (vs == 1) {
        const uint8_t *row = p + (long long)y * pitch;
        if (dw <= 2) return row[i];
        return (3 * row[i] + row[in] + (odd ? 2 : 1)) >> 2;
    }
    const int j = y >> 1;
    const uint8_t *row = p + (long long)j * pitch;
    if (dw <= 2) return row[i];
    const uint8_t *nrow = p + (long long)((y & 1) ? min(j + 1, dh - 1) : max(j - 1, 0)) * pitch;
    const int si = 3 * row[i] + nrow[i], sn = 3 * row[in] + nrow[in];
    return (3 * si + sn + (odd ? 7 : 8)) >> 4;
}

// A lane owns 4 consecutive pixels of the image's flattened [H * W] order: 12 bytes, three dword stores.  The last run of
// an image whose pixel count is no multiple of 4 stores bytes.
__global__ __launch_bounds__(JP_THREADS) void jpeg_color_kernel(const JDesc *__restrict__ desc, int B,
                                                                const uint8_t *__restrict__ ws, unsigned long long ws_bytes)
{
    const long long total = desc[B - 1].run_first + jp_runs(desc[B - 1]);
    const long long span = jp_span(total, JP_THREADS), begin = (long long)blockIdx.x * span, end = min(total, begin + span);
    JDesc d = {};
    long long nr = 0;
    for (long long u = begin + threadIdx.x; u < end; u += JP_THREADS) {
        if (u < d.run_first || u - d.run_first >= nr) {       // a contiguous span: the owner changes rarely
            d = desc[ragged_owner<true>(desc, B, u)];
            nr = jp_runs(d);
        }
        const long long lu = u - d.run_first, npx = (long long)d.H * d.W, nb = jp_blocks(d);
        if (lu < 0 || lu >= nr || d.plane_off < 0 || (unsigned long long)d.plane_off + (unsigned long long)nb * 64 > ws_bytes) continue;
        const int ypitch = d.mcus_x * d.hmax * 8, cpitch = d.mcus_x * 8;
        const uint8_t *py = ws + d.plane_off;
        const uint8_t *pcb = py + blocks_before(d, 1) * 64, *pcr = py + blocks_before(d, 2) * 64;
        const int dw = (d.W + d.hmax - 1) / d.hmax, dh = (d.H + d.vmax - 1) / d.vmax;
        const long long p0 = lu * 4;
        int y = (int)(p0 / d.W), x = (int)(p0 % d.W);
        unsigned char px[12];
        const int n = (int)min(4ll, npx - p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int R = 0, G = 0, Bl = 0;
            if (k < n) {
                const int Y = py[(long long)y * ypitch + x];
                if (d.ncomp == 1) {
                    R = G = Bl = Y;
                } else {
                    const int cb = jp_chroma(pcb, cpitch, dw, dh, d.hmax, d.vmax, y, x) - 128;
                    const int cr = jp_chroma(pcr, cpitch, dw, dh, d.hmax, d.vmax, y, x) - 128;
                    R = jp_clamp255(Y + ((91881 * cr + 32768) >> 16));
                    G = jp_clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                    Bl = jp_clamp255(Y + ((116130 * cb + 32768) >> 16));
                }
                if (++x == d.W) { x = 0; ++y; }
            }
            px[3 * k] = (unsigned char)R; px[3 * k + 1] = (unsigned char)G; px[3 * k + 2] = (unsigned char)Bl;
        }
        uint8_t *o = d.out + lu * 12;
        if (n == 4) {
            unsigned *o4 = (unsigned *)o;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
        } else {
            for (int k = 0; k < 3 * n; ++k) o[k] = px[k];
        }
    }
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_jpeg_workspace_bytes(const void *desc_host, int B)
{
    const BatchSize s = check_descriptors<JDesc>("mmr_jpeg_workspace_bytes", "decode", desc_host, B, true, jp_runs, [](const JDesc &e, int i) {
        if (e.out && !((uintptr_t)e.out & 3) && offsets_aligned(e)) return true;
        set_error("mmr_jpeg_workspace_bytes: descriptor %d: out must be 4-byte aligned, the offsets non-negative multiples of 16", i);
        return false;
    });
    return s.ok ? (size_t)(s.need ? s.need : 16) : 0;
}

extern "C" int mmr_jpeg_decode_device(const void *desc_dev, int B, const int16_t *coef_dev, const uint16_t *qt_dev, void *ws,
                                      size_t ws_bytes, void *stream)
{
    MMR_CHECK_ARG(B >= 0 && B <= 65535, "mmr_jpeg_decode_device: B=%d outside [0, 65535]", B);
    if (B == 0) return MMR_OK;
    MMR_CHECK_ARG(desc_dev && coef_dev && qt_dev && ws, "mmr_jpeg_decode_device: null pointer");
    MMR_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)qt_dev & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0,
                  "mmr_jpeg_decode_device: ws, coef_dev and qt_dev must be 16-byte aligned, the descriptors 8-byte aligned");
    MMR_CHECK_ARG(sizeof(JDesc) == 80, "mmr_jpeg_decode_device: descriptor layout drifted");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    // fixed grids: the sizes live in device memory.  The planes hold 64 bytes per block and at least one byte per pixel, which
    // bounds the work from ws_bytes; each workgroup takes a contiguous span of it and leaves at once when there is less.
    const unsigned long long max_blocks = ws_bytes / 64, max_runs = ws_bytes / 4 + (unsigned long long)B;
    const unsigned long long g1 = (max_blocks + JP_WAVES * 8 - 1) / (JP_WAVES * 8), g2 = (max_runs + JP_THREADS - 1) / JP_THREADS;
    const JDesc *d = (const JDesc *)desc_dev;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(grid_cap((unsigned)(g1 < 1 ? 1 : (g1 > JP_MAX_GRID ? JP_MAX_GRID : g1)))), dim3(JP_THREADS), 0, st, d, B,
                       (const uint8_t *)coef_dev, (const uint8_t *)qt_dev, (uint8_t *)ws, (unsigned long long)ws_bytes);
    MMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_color_kernel, dim3(grid_cap((unsigned)(g2 < 1 ? 1 : (g2 > JP_MAX_GRID ? JP_MAX_GRID : g2)))), dim3(JP_THREADS), 0, st, d, B,
                       (const uint8_t *)ws, (unsigned long long)ws_bytes);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
