// The body of deep_rescore_kernel (deep_topk.hip) and deep_rescore_qm_kernel (deep_qmask.hip), included INSIDE each kernel's
// braces (a text include, as sweep_scan_body.inc: as an inlined function the existing kernel compiled to a different
// instruction order).  In scope at the include: the kernel's template parameters T and PER, its arguments, and
// `constexpr bool QM` with `row_masks` / `mask_stride`: QM adds the listed pair's query's mask row,
// row_masks + query * mask_stride, to the liveness test (row_mask, nullable, stays the mask all queries share).
// One wave per listed pair, four rows per step (16 lanes each, quad_dot).  Survivors are appended as the sort's pair
// (query << 32 | row, ~ord_f64(dot64)); counter[1] keeps counting past the capacity.  A NaN dot fails the comparison.
    constexpr int E = PER * 64;
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    const unsigned long long nc = counter[0];
    const int64_t n = nc < (unsigned long long)tile_cap ? (int64_t)nc : tile_cap;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += (int64_t)gridDim.x * 4) {
        const uint64_t key = tiles[i];
        const int64_t qi = (int64_t)(key >> 32), base = (int64_t)(key & 0xffffffffu) * tile_rows;
        QuadQuery<T, PER> qq;
        qq.load(q + (size_t)qi * E, m);
        const double thr = thr_exact[qi];
#pragma unroll 2
        for (int r0 = 0; r0 < tile_rows; r0 += 4) {
            const int64_t row = base + r0 + g;
            bool live = row < N;
            const int64_t lrow = live ? row : N - 1;          // rows past N re-read the last row and are dropped
            if (row_mask) live = live && ((row_mask[lrow >> 5] >> (lrow & 31)) & 1u);
            if constexpr (QM) live = live && ((row_masks[(size_t)qi * mask_stride + (lrow >> 5)] >> (lrow & 31)) & 1u);
            QuadRow<T, PER> gr;
            gr.load(gal + (size_t)lrow * E, m);
            const double s = quad_dot<T, PER>(qq, gr);
            const bool keep = live && m == 0 && s >= thr;
            const uint64_t mask = __ballot(keep);
            if (mask) {
                unsigned long long wbase = 0;
                if (lane == 0) wbase = atomicAdd(counter + 1, (unsigned long long)__popcll(mask));
                wbase = __shfl(wbase, 0, 64);
                const unsigned long long pos = wbase + __popcll(mask & below);
                if (keep && pos < (unsigned long long)surv_cap) {
                    surv_k[pos] = ((uint64_t)qi << 32) | (uint64_t)row;
                    // ascending in this key = descending in dot64.  A dot64 of -0.0 cannot occur (every partial sum starts
                    // from +0.0 and round-to-nearest never turns a sum into -0.0), so equal dots have equal keys.
                    surv_o[pos] = ~ord_f64(s);
                }
            }
        }
    }
