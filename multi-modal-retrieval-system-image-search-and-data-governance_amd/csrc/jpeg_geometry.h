// The layout every JPEG stage agrees on, stated once: the zigzag table, the samplings and MCU grids in scope, the block
// counts, where a block of an image lies, and the order in which a scan visits the blocks.  The host coders, the kernels
// (through jpeg_device.h and jpeg_entropy_core.h) and the stand-alone sanitizer programs under tests/ take it from here.
// Plain C++ for host and device: nothing but <stdint.h>, no HIP call.
//
// An image is ncomp components (1: grey, 3: Y Cb Cr) on mcus_x x mcus_y MCUs; luma has hmax x vmax blocks per MCU, a chroma
// component one.  Coefficients (128 bytes a block) and planes (64 bytes a block) lie component after component, each in
// raster order over its padded block grid.  `g` below is any struct with the fields ncomp, hmax, vmax, mcus_x, mcus_y (and
// W, H where sizes are checked): the descriptors and mmr_jpeg_info of mmr.h, the host decoder's Parsed, the entropy kernel's Geo.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline __attribute__((always_inline))      // __forceinline__, without the HIP headers
#else
#define JPEG_HD inline
#endif

// zigzag position -> natural (row-major) position.  A macro so that it can initialise a host array and a __constant__ one.
#define JPEG_NATURAL_ORDER                                                                                                      \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

namespace mmr_jpeg {

// Grey at 1 x 1, or Y Cb Cr with luma at 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0) and chroma at 1 x 1: for three
// components those three pairs are exactly hmax in 1..2 with vmax in 1..hmax.
JPEG_HD bool sampling_in_scope(int ncomp, int hmax, int vmax)
{
    return ncomp == 1 ? (hmax == 1 && vmax == 1) : (ncomp == 3 && hmax >= 1 && hmax <= 2 && vmax >= 1 && vmax <= hmax);
}

// MCUs along a side of `side` pixels at luma sampling s
JPEG_HD int mcus_along(int side, int s) { return (side + 8 * s - 1) / (8 * s); }

// sides within 1..max_side and the MCU grid the one that covers them (for a sampling in scope)
template <class G>
JPEG_HD bool grid_in_scope(const G &g, int max_side)
{
    return g.W >= 1 && g.H >= 1 && g.W <= max_side && g.H <= max_side && g.mcus_x == mcus_along(g.W, g.hmax) && g.mcus_y == mcus_along(g.H, g.vmax);
}

// blocks of the components in front of component c (c = 3: of the whole image); of component c alone; of the image
template <class G>
JPEG_HD long long blocks_before(const G &g, int c)
{
    const long long mcus = (long long)g.mcus_x * g.mcus_y;
    return c == 0 ? 0 : mcus * g.hmax * g.vmax + (g.ncomp == 3 ? (c - 1) * mcus : 0);
}
template <class G>
JPEG_HD long long component_blocks(const G &g, int c) { return blocks_before(g, c + 1) - blocks_before(g, c); }
template <class G>
JPEG_HD long long image_blocks(const G &g) { return blocks_before(g, 3); }

struct BlockAt {
    int c, bw;                  // component; width of its plane in blocks
    long long at, plane;        // position within the component, in the caller's units; byte offset of its plane in the image's
};

// Position i within an image -> where it lies.  Positions count `unit` per block: 1 for block ordinals, 64 for plane bytes.
template <class G>
JPEG_HD BlockAt locate(const G &g, long long i, int unit)
{
    const long long cb = blocks_before(g, 1) * unit, cr = blocks_before(g, 2) * unit;
    if (i < cb) return {0, g.mcus_x * g.hmax, i, 0};
    const long long first = i >= cr ? cr : cb;
    return {i >= cr ? 2 : 1, g.mcus_x, i - first, first * (64 / unit)};
}

// The blocks of MCU m that belong to component c, in coding order: visit(block within the component's grid) for each,
// until one returns false; true if none did.
template <class G, class Visit>
inline bool mcu_blocks(const G &g, int64_t m, int c, Visit visit)
{
    const int h = c == 0 ? g.hmax : 1, v = c == 0 ? g.vmax : 1;
    const int64_t mx = m % g.mcus_x, my = m / g.mcus_x, bw = (int64_t)g.mcus_x * h;
    for (int by = 0; by < v; ++by)
        for (int bx = 0; bx < h; ++bx)
            if (!visit((my * v + by) * bw + mx * h + bx)) return false;
    return true;
}

}  // namespace mmr_jpeg
