// Train-time augmentation, part 1: the bicubic coefficient tables of B random crops, built on the device.
//
// The reference's few-shot loader applies RandomResizedCrop(224, BICUBIC) + RandomHorizontalFlip per image per epoch
// (reference code/custom.py:24-29).  Every random crop has its own size, so the host table builder
// (preprocess.resample_tables, a Python loop per output coordinate) would run once per crop per axis and its cache would
// never hit.  Here one launch builds both tables of every crop: one thread per (crop, axis, output coordinate), a
// sequential loop over its taps, every double operation rounded to nearest and never fused (augment_tables.h) -- the same
// integers as Pillow's precompute_coeffs + normalize_coeffs_8bpc.  A flipped crop gets its horizontal rows in reverse
// order, which is all a horizontal flip after the resize amounts to.  mmr_augment_resample (preprocess.hip) applies them.
#pragma clang fp contract(off)

#include "mmr_common.h"
#include "augment_tables.h"

namespace mmr {

__global__ __launch_bounds__(256) void augment_tables_kernel(const CropDesc *__restrict__ desc, int B, int S, int kmax,
                                                             int32_t *__restrict__ tables)
{
    const int b = blockIdx.y;
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= 2 * S) return;
    const int axis = id / S, j = id - axis * S;
    const CropDesc d = desc[b];
    const int in = axis == 0 ? d.cw : d.ch;
    int32_t *bound = const_cast<int32_t *>(aug_bounds(tables, b, axis, S)) + 2 * j;
    int32_t *row = const_cast<int32_t *>(aug_coeffs(tables, B, b, axis, S, kmax)) + (size_t)j * kmax;
    if (in < 1 || in > AUG_IN_MAX || aug_ksize(in, S) > kmax) {     // not a crop these tables can hold: an empty row
        bound[0] = 0;
        bound[1] = 0;
        for (int x = 0; x < kmax; ++x) row[x] = 0;
        return;
    }
    aug_table_row(in, S, (axis == 0 && d.flip) ? S - 1 - j : j, kmax, bound, row);
}

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_augment_tables_bytes(int B, int S, int kmax)
{
    if (B < 0 || S < 1 || kmax < 1) return 0;
    return aug_tables_bytes(B, S, kmax);
}

extern "C" int mmr_augment_tables(const void *desc, int B, int S, int kmax, void *tables, size_t tables_bytes, void *stream)
{
    MMR_CHECK_ARG(desc && tables, "mmr_augment_tables: null pointer");
    MMR_CHECK_ARG(B >= 0 && B <= 65535 && S >= 1 && S <= 4096, "mmr_augment_tables: bad size B=%d S=%d", B, S);
    MMR_CHECK_ARG(kmax >= 8 && kmax % 4 == 0 && kmax <= 4 * AUG_IN_MAX, "mmr_augment_tables: kmax=%d is not a padded ksize", kmax);
    MMR_CHECK_ARG(((uintptr_t)tables & 15) == 0, "mmr_augment_tables: tables not 16-byte aligned");
    MMR_CHECK_ARG(tables_bytes >= aug_tables_bytes(B, S, kmax), "mmr_augment_tables: %zu table bytes, need %zu", tables_bytes,
                  aug_tables_bytes(B, S, kmax));
    MMR_CHECK_ARG(sizeof(CropDesc) == 48, "mmr_augment_tables: descriptor layout drifted");
    if (B == 0) return MMR_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    hipLaunchKernelGGL(augment_tables_kernel, dim3((2 * S + 255) / 256, B), dim3(256), 0, st, (const CropDesc *)desc, B, S, kmax,
                       (int32_t *)tables);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
