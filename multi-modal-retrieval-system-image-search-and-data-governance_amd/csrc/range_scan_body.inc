// The body of range_scan_kernel (range.hip, bf16 operands) and range_scan_f16_kernel (range_f16.hip), included INSIDE each
// kernel's braces.  In scope at the include: the kernel's template parameters (E, TRI, MASKED), its argument `RangeScanArgs a`, and
// `using ET = bf16_t` or `f16_t`, the element type behind a.q / a.gal -- it picks the MFMA instruction (scan_pipeline.h)
// and how the resident query's norm is read; everything else is the same text.  A text include and not a function: as
// an inlined function the bf16 kernels compiled to slightly different instruction streams than before the fp16 forms
// existed (register allocation and scalar-load order); as the kernel's own statements they compile bit for bit.
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    // work item -> (first query id, tile range)
    int64_t qbase;
    int t0, t1;
    if constexpr (TRI) {
        const int64_t w = blockIdx.x, F = a.fblk;
        int64_t b, ch;
        if (a.order == 0) {
            int64_t lo = 0, hi = a.nchunk - 1;          // largest chunk with S(chunk) <= w
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (tri_items_before_chunk(mid, a.nblk, F) <= w) lo = mid; else hi = mid - 1;
            }
            ch = lo;
            b = w - tri_items_before_chunk(ch, a.nblk, F);
        } else {
            int64_t lo = 0, hi = a.nblk - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (tri_items_before_block(mid, a.nchunk, F) <= w) lo = mid; else hi = mid - 1;
            }
            b = lo;
            ch = b / F + (w - tri_items_before_block(b, a.nchunk, F));
        }
        qbase = b * C::QMAX;
        const int64_t first = qbase / RTILE;          // the tile that holds row b*QMAX
        t0 = (int)max((int64_t)ch * RTRI_TPC, first);
        t1 = (int)min((int64_t)a.ntiles, (int64_t)(ch + 1) * RTRI_TPC);
    } else {
        qbase = a.q0;
        t0 = blockIdx.x * a.tpt;
        t1 = min(a.ntiles, t0 + a.tpt);
    }
    const int64_t nq = TRI ? N : (int64_t)a.q0 + a.Qc;   // query ids below this are live

    // B operand: this wave's 32 queries (scan_kernel's layout)
    const int64_t gq = qbase + wave * 32 + c;
    bool qlive = gq < nq;
    const bool compute = TRI ? qbase + wave * 32 < N : wave * 32 < a.Qc;   // wave-uniform: this wave holds a live query
    // mask words of the tiles [t0, t1) (at most RMAX_TPT / RTRI_TPC = 64) and, in the self-join, the query row's own word:
    // issued in front of the query loads, taken behind them (scan_pipeline.h: mask_issue)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    const MaskWord mq = MASKED && TRI ? mask_issue(a.row_mask, (qlive ? gq : 0) >> 5, 64, 0) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    double qn2 = 0.0;                  // fp64: a small query's squares underflow in fp32
    {
        const bf16_t *qp = TRI ? a.gal + (size_t)(qlive ? gq : 0) * E + h * 8
                               : a.q + (size_t)(qlive ? gq - a.q0 : 0) * E + h * 8;
        load_query_b16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = b16_to_f32<ET>((uint16_t)bq[s][j]); qn2 += x * x; }
    }
    qn2 += __shfl_xor(qn2, 32, 64);
    const uint32_t mwords = mask_take(mw);
    if constexpr (MASKED && TRI) qlive = qlive && ((mask_take(mq) >> (gq & 31)) & 1u);   // a masked query row is not live

    // this lane's candidate threshold: threshold - margin(query) (range_common.h), rounded down to fp32
    float thr;
    bool wild;
    {
        const ScanMargin mg = scan_margin(qn2, a.host_bound, a.dev_bound, a.split, a.resid_dev, a.qres, qlive ? gq : 0);
        wild = mg.wild;
        const double lo = wild ? -INFINITY : a.threshold - mg.eps;
        thr = (float)lo;
        if ((double)thr > lo) thr = nextafterf(thr, -INFINITY);
    }

    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.gal, a.gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [] {},
        [&](int t, int cur) {
            if (!compute) return;
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(query gq, row t*32 + (i&3) + 8*(i>>2) + 4h)
            const int64_t base = (int64_t)t * RTILE + 4 * h;
            const uint32_t wh = MASKED ? row_mask_tile32(mwords, t, t0, N) >> (4 * h) : 0u;
            uint32_t pred = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t r = base + (i & 3) + 8 * (i >> 2);
                const bool p = qlive && (MASKED ? ((wh >> ((i & 3) + 8 * (i >> 2))) & 1u) : r < N) && (acc[i] >= thr || wild) &&
                               (!TRI || r > gq);
                pred |= p ? (1u << i) : 0u;
            }
            append_candidates(pred, lane, a.counter, a.cand, a.cand_cap, (uint64_t)gq << 32, base);
        });
