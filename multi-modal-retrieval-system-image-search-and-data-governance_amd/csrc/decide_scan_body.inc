// The body of decide_scan_kernel (decide.hip, bf16 operands) and decide_scan_f16_kernel (decide_f16.hip), included INSIDE
// each kernel's braces, like range_scan_body.inc.  In scope at the include: the kernel's template parameters (E, MASKED),
// its argument `DecideScanArgs a`, and `using ET = bf16_t` or `f16_t`, the element type behind a.q / a.gal.
// range_scan_kernel's non-TRI structure with a deciding epilogue: a 32-row tile is one mask word per query.
    using C = RangeCfg<E>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t N = a.N;

    const int t0 = blockIdx.x * a.tpt;
    const int t1 = min(a.ntiles, t0 + a.tpt);
    const int64_t nq = (int64_t)a.q0 + a.Qc;              // query ids below this are live

    // B operand: this wave's 32 queries (scan_kernel's layout)
    const int64_t gq = (int64_t)a.q0 + wave * 32 + c;
    const bool qlive = gq < nq;
    const bool compute = wave * 32 < a.Qc;                // wave-uniform: this wave holds a live query
    // mask words of the tiles [t0, t1): issued in front of the query loads, taken behind them (scan_pipeline.h: mask_issue)
    const MaskWord mw = MASKED ? mask_issue(a.row_mask, t0, t1 - t0, lane) : MaskWord{0u, false};
    bf16x8 bq[C::KSTEPS];
    double qn2 = 0.0;                  // fp64: a small query's squares underflow in fp32
    {
        const bf16_t *qp = a.q + (size_t)(qlive ? gq - a.q0 : 0) * E + h * 8;
        load_query_b16<C::KSTEPS, 16>(qp, qlive, bq);
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = b16_to_f32<ET>((uint16_t)bq[s][j]); qn2 += x * x; }
    }
    qn2 += __shfl_xor(qn2, 32, 64);
    const uint32_t mwords = mask_take(mw);

    // this lane's two thresholds: an approximate dot at or above thr_hi is a certain pass, one below thr_lo a certain
    // fail (|acc - dot64| <= eps: range_common.h), anything else -- NaN included -- is left to the fp64 recheck.  A wild
    // query, or one whose threshold is not finite, leaves every pair to it.
    float thr_lo, thr_hi;
    {
        const ScanMargin mg = scan_margin(qn2, a.host_bound, a.dev_bound, a.split, a.resid_dev, a.qres, qlive ? gq : 0);
        const double thr = a.thresholds[qlive ? gq : 0];
        const bool wild = mg.wild || !(fabs(thr) < INFINITY);
        // a wild lane compares against NaN: no element is a certain pass, none a certain fail, every pair is open
        thr_lo = wild ? NAN : f32_down(thr - mg.eps);
        thr_hi = wild ? NAN : f32_up(thr + mg.eps);
    }

    PendingWord pw{a.out + (size_t)(qlive ? gq : 0) * a.ntiles, compute && qlive && h == 0};

    tile_ring<RNBUF, C::LPW>(
        t0, t1, [&](int tile, int buf) { stage_tile<C>(a.gal, a.gal, N, tile, smem + buf * C::TILE_BYTES, wave, lane); },
        [&] { pw.flush(); },
        [&](int t, int cur) {
            if (!compute) return;
            const f32x16 acc = tile_dot_32x32<E, chains_32x32(C::WAVES), RPF, ET>(smem + cur * C::TILE_BYTES + c * C::ROWB, c, h, bq);

            // epilogue: acc[i] = dot(query gq, row t*32 + (i&3) + 8*(i>>2) + 4h), bit (i&3) + 8*(i>>2) + 4h of the word
            const int64_t base = (int64_t)t * RTILE + 4 * h;
            const int64_t left = N - (int64_t)t * RTILE;
            const uint32_t lw = MASKED ? row_mask_tile32(mwords, t, t0, N) : (left < 32 ? (1u << (int)left) - 1u : 0xffffffffu);
            const uint32_t wh = lw >> (4 * h);
            // pass: certain passes; alive: everything but the certain fails (NaN included); both at the rows' bit positions
            uint32_t pass = 0, alive = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t bit = 1u << ((i & 3) + 8 * (i >> 2));
                pass |= acc[i] >= thr_hi ? bit : 0u;
                alive |= acc[i] < thr_lo ? 0u : bit;
            }
            // open pairs of live rows of a live query, moved from bit (i&3) + 8*(i>>2) to bit i for append_candidates
            const uint32_t ob = qlive ? (alive & ~pass & wh) : 0u;
            const uint32_t pred = (ob & 0xfu) | ((ob >> 4) & 0xf0u) | ((ob >> 8) & 0xf00u) | ((ob >> 12) & 0xf000u);
            append_candidates(pred, lane, a.counter, a.cand, a.cand_cap, (uint64_t)gq << 32, base);
            pass <<= 4 * h;
            pass |= __shfl_xor(pass, 32, 64);
            pw.set(t, pass & lw);
        });
    pw.flush();
