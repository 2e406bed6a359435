// The Huffman stage of the JPEG decode on the device (the contract is in mmr.h, the algorithm and its proof obligations in
// jpeg_entropy_core.h, which this file and the CPU emulation share).  One workgroup owns one image and no wave ever waits
// on another workgroup; the only synchronisation is __syncthreads().
//   1. zero-fill the coefficient span; Huffman tables -> LDS; every subsequence gets its default entry state
//   2. rounds: (a) each lane decodes the subsequences whose entry state changed, keeping exit state and block count;
//      (b) exits become the next entries; until a round changes nothing, at most max_rounds times
//   3. prefix sum of the block counts -> the ordinal of every subsequence's first block
//   4. final pass: decode from the converged states under the host stage's rules, write coefficients (DC as differences)
//   5. DC pass: per-component running sums over the MCUs, reset at restart intervals
// Loop bounds: rounds <= max_rounds <= 1024; a subsequence takes at most 8 S + 31 steps; everything else runs over
// counts taken from the descriptor.  States live in LDS up to JE_LDS_SUBSEQ subsequences, beyond that in `ws`.
#include "mmr_common.h"

#include "jpeg_entropy_core.h"

namespace mmr {

using namespace mmr_jpe;

constexpr int JE_THREADS = JPE_LANES;   // 16 waves a workgroup: the decode is a chain of dependent loads, more waves hide them
constexpr int JE_LDS_SUBSEQ = 2048;
constexpr uint32_t JE_DIRTY = 0x80000000u;

typedef mmr_jpeg_scan_desc SDesc;

__constant__ uint8_t je_natural[64] = JPE_NATURAL_ORDER;

__device__ __forceinline__ uint32_t je_aux(const Run &r) { return (uint32_t)r.idx | ((uint32_t)r.slot << 6); }

__global__ __launch_bounds__(JE_THREADS) void jpeg_entropy_kernel(const SDesc *__restrict__ desc, int B, const uint8_t *__restrict__ bytes,
                                                                  const uint8_t *__restrict__ tables, uint8_t *__restrict__ coef_base,
                                                                  int32_t *__restrict__ stat, int S, int max_rounds, uint8_t *ws,
                                                                  unsigned long long ws_bytes)
{
    __shared__ uint32_t s_tab[JPE_TABLES * JPE_TABLE_WORDS];
    __shared__ uint32_t s_state[4 * JE_LDS_SUBSEQ];
    __shared__ uint32_t s_part[JE_THREADS];
    __shared__ uint32_t s_dc[3 * JE_THREADS];     // a lane's DC sum (16 bits) | JE_DIRTY if its range holds a restart
    __shared__ uint8_t s_nat[64];
    __shared__ int s_changed, s_bad, s_done;

    const int img = blockIdx.x, tid = threadIdx.x;
    if (img >= B) return;
    const SDesc d = desc[img];
    Geo G;
    const int dcs[3] = {d.td0, d.td1, d.td2}, acs[3] = {d.ta0, d.ta1, d.ta2};
    const bool empty = d.status != 0 || d.ncomp == 0;
    const bool usable = !empty && jpe_geo(G, d.ncomp, d.hmax, d.vmax, d.mcus_x, d.mcus_y, d.restart, dcs, acs) && d.scan_bytes >= 1 &&
                        d.scan_bytes <= MMR_JPEG_DEVICE_MAX_SCAN && d.bytes_off >= 0 && d.tables_off >= 0 && d.coef_off >= 0 &&
                        G.blocks[0] == (uint32_t)d.blocks0 && G.blocks[1] == (uint32_t)d.blocks1 && G.blocks[2] == (uint32_t)d.blocks2;
    const uint32_t nbytes = usable ? (uint32_t)d.scan_bytes : 0u;
    const uint32_t nsub = usable ? (nbytes + (uint32_t)S - 1u) / (uint32_t)S : 0u;
    const bool in_lds = nsub <= (uint32_t)JE_LDS_SUBSEQ;
    const bool fits = in_lds || (d.state_off >= 0 && (unsigned long long)d.state_off + 16ull * nsub <= ws_bytes);
    if (!usable || !fits) {                  // uniform over the workgroup: nobody meets a barrier
        if (tid == 0) {
            stat[4 * img + 0] = empty && d.status != 0 ? d.status : MMR_JPEG_DECLINED;
            stat[4 * img + 1] = 0;
            stat[4 * img + 2] = (int32_t)nsub;
            stat[4 * img + 3] = 0;
        }
        return;
    }
    uint32_t *st = in_lds ? s_state : (uint32_t *)(ws + d.state_off);
    uint32_t *e_pos = st, *e_aux = st + nsub, *x_pos = st + 2 * (size_t)nsub, *x_aux = st + 3 * (size_t)nsub;
    int16_t *coef = (int16_t *)(coef_base + d.coef_off);
    const Scan scan = {(const uint32_t *)(bytes + d.bytes_off), nbytes};
    const int max_steps = 8 * S + 31;

    // 1. zero-fill, tables, default entries
    {
        uint4 *z = (uint4 *)coef;
        const uint4 zero = {0u, 0u, 0u, 0u};
        for (uint32_t i = tid; i < G.total * 8u; i += JE_THREADS) z[i] = zero;
        const uint32_t *t = (const uint32_t *)(tables + d.tables_off);
        for (int i = tid; i < JPE_TABLES * JPE_TABLE_WORDS; i += JE_THREADS) s_tab[i] = t[i];
        if (tid < 64) s_nat[tid] = je_natural[tid];
        for (uint32_t k = tid; k < nsub; k += JE_THREADS) {
            e_pos[k] = k ? jpe_default_pos(scan, k, (uint32_t)S) : 0u;
            e_aux[k] = JE_DIRTY;
        }
        if (tid == 0) { s_bad = 0; s_done = 0; }
    }
    __syncthreads();

    // 2. rounds
    int rounds = 0;
    bool converged = false;
    while (rounds < max_rounds && !converged) {
        ++rounds;
        if (tid == 0) s_changed = 0;
        for (uint32_t k = tid; k < nsub; k += JE_THREADS) {
            const uint32_t aux = e_aux[k];
            if (!(aux & JE_DIRTY)) continue;
            Run r;
            r.pos = e_pos[k]; r.idx = (int)(aux & 63u); r.slot = (int)((aux >> 6) & 7u);
            const uint32_t end_bits = (k + 1u) * (uint32_t)S < nbytes ? (k + 1u) * (uint32_t)S * 8u : nbytes * 8u;
            jpe_run<false>(scan, s_tab, G, s_nat, end_bits, max_steps, r, 0u, nullptr);
            x_pos[k] = r.pos;
            x_aux[k] = je_aux(r) | (r.blocks << 16);
            e_aux[k] = aux & ~JE_DIRTY;
        }
        __syncthreads();
        for (uint32_t k = tid; k + 1u < nsub; k += JE_THREADS) {
            const uint32_t xp = x_pos[k], xa = x_aux[k] & 0x1FFu;
            if (xp != e_pos[k + 1] || xa != (e_aux[k + 1] & 0x1FFu)) {
                e_pos[k + 1] = xp;
                e_aux[k + 1] = xa | JE_DIRTY;
                s_changed = 1;
            }
        }
        __syncthreads();
        converged = s_changed == 0;
        __syncthreads();                     // everyone has read s_changed before the next round clears it
    }

    if (converged) {
        // 3. exclusive prefix sum of the block counts, into x_pos: each lane owns a contiguous range of subsequences
        const uint32_t per = (nsub + JE_THREADS - 1u) / JE_THREADS;
        const uint32_t k0 = min((uint32_t)tid * per, nsub), k1 = min(k0 + per, nsub);
        uint32_t sum = 0;
        for (uint32_t k = k0; k < k1; ++k) sum += x_aux[k] >> 16;
        s_part[tid] = sum;
        __syncthreads();
        uint32_t g = 0;
        for (int j = 0; j < tid; ++j) g += s_part[j];
        for (uint32_t k = k0; k < k1; ++k) {
            x_pos[k] = g;
            g += x_aux[k] >> 16;
        }
        __syncthreads();

        // 4. final pass
        int bad = 0, done = 0;
        for (uint32_t k = tid; k < nsub; k += JE_THREADS) {
            const uint32_t aux = e_aux[k], g0 = x_pos[k];
            Run r;
            r.pos = e_pos[k]; r.idx = (int)(aux & 63u); r.slot = (int)((aux >> 6) & 7u);
            const uint32_t end_bits = (k + 1u) * (uint32_t)S < nbytes ? (k + 1u) * (uint32_t)S * 8u : nbytes * 8u;
            jpe_run<true>(scan, s_tab, G, s_nat, end_bits, max_steps, r, g0, coef);
            bad |= r.bad;
            done += r.done;
            if (!r.bad && k + 1u < nsub &&
                (r.pos != e_pos[k + 1] || je_aux(r) != (e_aux[k + 1] & 0x1FFu) || g0 + r.blocks != x_pos[k + 1]))
                bad = 1;
        }
        if (bad) atomicOr(&s_bad, 1);
        if (done) atomicAdd(&s_done, done);
        __syncthreads();                     // also orders the coefficient stores in front of the DC pass's loads
    }
    const bool good = converged && s_bad == 0 && s_done == 1;

    if (good) {
        // 5. DC pass: each lane owns a contiguous range of MCUs
        const uint32_t mcus = (uint32_t)G.mcus_x * (uint32_t)G.mcus_y, per = (mcus + JE_THREADS - 1u) / JE_THREADS;
        const uint32_t m0 = min((uint32_t)tid * per, mcus), m1 = min(m0 + per, mcus);
        for (int c = 0; c < G.ncomp; ++c) {
            uint32_t sum = 0;
            int reset = 0;
            jpe_dc_range(G, c, m0, m1, coef, false, sum, reset);
            s_dc[c * JE_THREADS + tid] = sum | (reset ? JE_DIRTY : 0u);
        }
        __syncthreads();
        for (int c = 0; c < G.ncomp; ++c) {
            uint32_t sum = 0;
            for (int j = 0; j < tid; ++j) {
                const uint32_t part = s_dc[c * JE_THREADS + j];
                sum = ((part & JE_DIRTY ? 0u : sum) + part) & 0xFFFFu;
            }
            int reset = 0;
            jpe_dc_range(G, c, m0, m1, coef, true, sum, reset);
        }
    }
    if (tid == 0) {
        stat[4 * img + 0] = good ? MMR_JPEG_OK : MMR_JPEG_DECLINED;
        stat[4 * img + 1] = rounds;
        stat[4 * img + 2] = (int32_t)nsub;
        stat[4 * img + 3] = 0;
    }
}

static bool je_subseq_ok(int S) { return S >= 16 && S <= 1024 && (S & (S - 1)) == 0; }

}  // namespace mmr

using namespace mmr;

extern "C" size_t mmr_jpeg_entropy_workspace_bytes(const void *scan_desc_host, int B, int subseq_bytes)
{
    if (!scan_desc_host || B < 1 || B > 65535 || !je_subseq_ok(subseq_bytes)) {
        set_error("mmr_jpeg_entropy_workspace_bytes: %s", !scan_desc_host ? "null descriptor array"
                                                          : !je_subseq_ok(subseq_bytes) ? "subseq_bytes must be a power of two in 16..1024"
                                                                                        : "B outside [1, 65535]");
        return 0;
    }
    const SDesc *d = (const SDesc *)scan_desc_host;
    unsigned long long need = 16;
    for (int i = 0; i < B; ++i) {
        const SDesc &e = d[i];
        if (e.status != 0 || e.ncomp == 0) continue;
        Geo G;
        const int dcs[3] = {e.td0, e.td1, e.td2}, acs[3] = {e.ta0, e.ta1, e.ta2};
        if (!jpe_geo(G, e.ncomp, e.hmax, e.vmax, e.mcus_x, e.mcus_y, e.restart, dcs, acs) || G.blocks[0] != (uint32_t)e.blocks0 ||
            G.blocks[1] != (uint32_t)e.blocks1 || G.blocks[2] != (uint32_t)e.blocks2) {
            set_error("mmr_jpeg_entropy_workspace_bytes: descriptor %d: %d components, sampling %d x %d, %d x %d MCUs, restart %d or its "
                      "block counts or table slots are outside what the kernel decodes", i, e.ncomp, e.hmax, e.vmax, e.mcus_y, e.mcus_x, e.restart);
            return 0;
        }
        if (e.scan_bytes < 1 || e.scan_bytes > MMR_JPEG_DEVICE_MAX_SCAN) {
            set_error("mmr_jpeg_entropy_workspace_bytes: descriptor %d: scan_bytes %lld outside [1, %d]", i, (long long)e.scan_bytes, MMR_JPEG_DEVICE_MAX_SCAN);
            return 0;
        }
        if (e.bytes_off < 0 || (e.bytes_off & 15) || e.tables_off < 0 || (e.tables_off & 15) || e.coef_off < 0 || (e.coef_off & 15) ||
            e.state_off < 0 || (e.state_off & 15)) {
            set_error("mmr_jpeg_entropy_workspace_bytes: descriptor %d: the offsets must be non-negative multiples of 16", i);
            return 0;
        }
        const unsigned long long nsub = ((unsigned long long)e.scan_bytes + subseq_bytes - 1) / subseq_bytes;
        if (nsub > (unsigned long long)JE_LDS_SUBSEQ && (unsigned long long)e.state_off + 16 * nsub > need) need = (unsigned long long)e.state_off + 16 * nsub;
    }
    return (size_t)need;
}

extern "C" int mmr_jpeg_entropy_decode_device(const void *scan_desc_dev, int B, const void *bytes_dev, const void *tables_dev,
                                              int16_t *coef_dev, int32_t *stat_dev, int subseq_bytes, int max_rounds, void *ws,
                                              size_t ws_bytes, void *stream)
{
    MMR_CHECK_ARG(B >= 0 && B <= 65535, "mmr_jpeg_entropy_decode_device: B=%d outside [0, 65535]", B);
    MMR_CHECK_ARG(je_subseq_ok(subseq_bytes), "mmr_jpeg_entropy_decode_device: subseq_bytes=%d must be a power of two in 16..1024", subseq_bytes);
    MMR_CHECK_ARG(max_rounds >= 1 && max_rounds <= 1024, "mmr_jpeg_entropy_decode_device: max_rounds=%d outside [1, 1024]", max_rounds);
    if (B == 0) return MMR_OK;
    MMR_CHECK_ARG(scan_desc_dev && bytes_dev && tables_dev && coef_dev && stat_dev && ws, "mmr_jpeg_entropy_decode_device: null pointer");
    MMR_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)bytes_dev & 15) == 0 &&
                      ((uintptr_t)tables_dev & 15) == 0 && ((uintptr_t)scan_desc_dev & 7) == 0 && ((uintptr_t)stat_dev & 3) == 0,
                  "mmr_jpeg_entropy_decode_device: ws, coef_dev, bytes_dev and tables_dev must be 16-byte aligned, the descriptors 8-byte aligned");
    MMR_CHECK_ARG(sizeof(SDesc) == 112 && JPE_TABLES * JPE_TABLE_WORDS * 4 == MMR_JPEG_TABLE_BYTES, "mmr_jpeg_entropy_decode_device: descriptor or table layout drifted");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(MMR_PROF_ROWWISE, st);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)B), dim3(JE_THREADS), 0, st, (const SDesc *)scan_desc_dev, B, (const uint8_t *)bytes_dev,
                       (const uint8_t *)tables_dev, (uint8_t *)coef_dev, stat_dev, subseq_bytes, max_rounds, (uint8_t *)ws,
                       (unsigned long long)ws_bytes);
    MMR_CHECK_LAUNCH();
    return MMR_OK;
}
