// What the two device stages of the JPEG path (jpeg.hip: decode, jpeg_encode.hip: encode) share beyond the layout in
// jpeg_geometry.h: the owner search over a ragged batch, the constants of libjpeg's integer DCT, the per-wave LDS tile of
// the 8 x 8 transposes, and the descriptor checks of the two *_workspace_bytes calls.  Include after mmr_common.h.
#pragma once
#include "jpeg_geometry.h"

namespace mmr {

using namespace mmr_jpeg;

// jidctint / jfdctint, CONST_BITS 13: FIX(0.298631336) ... FIX(3.072711026)
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
              F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

// the largest i with first(desc[i]) <= g: rows without units share their successor's prefix and are never the answer
template <bool RUNS, class Desc>
__device__ __forceinline__ int ragged_owner(const Desc *__restrict__ desc, int B, long long g)
{
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((RUNS ? desc[mid].run_first : desc[mid].block_first) <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A wave transposes its 8 blocks of 8 x 8 ints through a tile of 64 rows, one per lane: lane 8 b + r holds row r of block b.
// A lane scatters or gathers its own row, or (COLUMN) column r of its block.  The caller puts a barrier between a scatter
// and the gather that follows it.
constexpr int TILE_STRIDE = 9;        // dwords per tile row: 8 + 1 pad, so that a column access touches 64 distinct banks
template <bool COLUMN>
__device__ __forceinline__ int tile_at(int lane, int k) { return COLUMN ? ((lane & ~7) + k) * TILE_STRIDE + (lane & 7) : lane * TILE_STRIDE + k; }
template <bool COLUMN>
__device__ __forceinline__ void tile_put(int *t, int lane, const int (&x)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) t[tile_at<COLUMN>(lane, k)] = x[k];
}
template <bool COLUMN>
__device__ __forceinline__ void tile_get(const int *t, int lane, int (&x)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t[tile_at<COLUMN>(lane, k)];
}

template <class Desc>
bool offsets_aligned(const Desc &e)
{
    return e.coef_off >= 0 && !(e.coef_off & 15) && e.qt_off >= 0 && !(e.qt_off & 15) && e.plane_off >= 0 && !(e.plane_off & 15);
}

struct BatchSize {
    bool ok;
    unsigned long long need;      // bytes of planes, up to the end of the last row's
    long long blocks, runs;
};

// The descriptor checks of `fn` (a *_workspace_bytes call, whose kernels `verb` images): prefix sums, scope, row_ok(e, i)
// for what only that descriptor type holds (it reports its own failures), planes that do not overlap.  skip_empty: a row
// with ncomp == 0 is passed over.  !ok: set_error has been called.
template <class Desc, class Runs, class RowOk>
BatchSize check_descriptors(const char *fn, const char *verb, const void *desc_host, int B, bool skip_empty, Runs runs_of, RowOk row_ok)
{
    BatchSize s = {false, 0, 0, 0};
    if (!desc_host || B < 1 || B > 65535) {
        set_error("%s: %s", fn, desc_host ? "B outside [1, 65535]" : "null descriptor array");
        return s;
    }
    const Desc *d = (const Desc *)desc_host;
    for (int i = 0; i < B; ++i) {
        const Desc &e = d[i];
        if (e.block_first != s.blocks || e.run_first != s.runs) {
            set_error("%s: descriptor %d: block_first / run_first are not the prefix sums of the rows before it", fn, i);
            return s;
        }
        if (skip_empty && e.ncomp == 0) continue;
        if (!sampling_in_scope(e.ncomp, e.hmax, e.vmax) || !grid_in_scope(e, MMR_JPEG_MAX_SIDE)) {
            set_error("%s: descriptor %d: %d x %d, %d components, sampling %d x %d, %d x %d MCUs is outside what the kernels %s", fn, i, e.H,
                      e.W, e.ncomp, e.hmax, e.vmax, e.mcus_y, e.mcus_x, verb);
            return s;
        }
        if (!row_ok(e, i)) return s;
        if ((unsigned long long)e.plane_off < s.need) {
            set_error("%s: descriptor %d: its planes overlap those of an earlier row", fn, i);
            return s;
        }
        s.blocks += image_blocks(e);
        s.runs += runs_of(e);
        s.need = (unsigned long long)e.plane_off + (unsigned long long)image_blocks(e) * 64;
    }
    s.ok = true;
    return s;
}

}  // namespace mmr
