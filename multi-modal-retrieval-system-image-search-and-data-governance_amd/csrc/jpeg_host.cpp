// Host stage of the JPEG decode: header parsing and the Huffman (entropy) stage of baseline / extended-sequential files,
// on up to 16 std::threads.  Plain C++17 with no HIP call: it also builds with g++ (tests/jpeg_fuzz_main.cpp runs it under
// the address and undefined-behaviour sanitizers).  The device stage is jpeg.hip; the contract of both is in mmr.h.
// mmr_jpeg_scan_prepare, at the end, is the host part of the optional device Huffman stage (jpeg_entropy.hip): headers only.
// The block layout and the order of a scan are jpeg_geometry.h's; error reporting and the thread pool jpeg_host_util.h's.
//
// Every read of the file goes through `pos < size` checks and every coefficient write through `k <= 63` and the block
// count the headers gave, so no input reads or writes outside its buffers.
#include <string.h>

#include "jpeg_host_util.h"

namespace {

using namespace mmr_jpeg;

const uint8_t kNatural[64] = JPEG_NATURAL_ORDER;

constexpr int OK = MMR_JPEG_OK, UNSUPPORTED = MMR_JPEG_UNSUPPORTED, CORRUPT = MMR_JPEG_CORRUPT;
constexpr int FAST = 9;   // codes of up to FAST bits decode by one table look-up

struct Huff {
    bool defined = false;
    uint8_t bits[17];      // bits[l]: codes of length l
    uint8_t vals[256];
    int32_t maxcode[18];   // largest code of length l, -1 for none
    int32_t delta[17];     // vals index = code + delta[l]
    uint16_t fast[1 << FAST];   // (length << 8) | symbol, 0: longer than FAST bits or undefined
};

struct Parsed {
    int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1, mcus_x = 0, mcus_y = 0, restart = 0;
    int h[3] = {1, 1, 1}, v[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, id[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint16_t qt[4][64];
    bool qt_defined[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int64_t scan = 0;      // offset of the first entropy-coded byte
};

// counts and symbols -> the decoding tables; false for counts that are no prefix code
bool huff_derive(Huff &t)
{
    int32_t code = 0, k = 0;
    memset(t.fast, 0, sizeof(t.fast));
    for (int l = 1; l <= 16; ++l) {
        t.delta[l] = k - code;
        for (int i = 0; i < t.bits[l]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;
            if (l <= FAST)
                for (int f = 0; f < (1 << (FAST - l)); ++f)
                    t.fast[(code << (FAST - l)) | f] = (uint16_t)((l << 8) | t.vals[k]);
        }
        t.maxcode[l] = t.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    return true;
}

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// Reads the markers up to and including the SOS header of the first scan.
int parse_headers(const uint8_t *d, int64_t n, Parsed &P)
{
    if (d == nullptr || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return CORRUPT;
    int64_t pos = 2;
    bool sof = false, adobe = false, jfif = false;
    int adobe_transform = 0;
    for (;;) {
        if (pos >= n || d[pos] != 0xFF) return CORRUPT;
        while (pos < n && d[pos] == 0xFF) ++pos;          // fill bytes
        if (pos >= n) return CORRUPT;
        const int m = d[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // parameterless
        if (m == 0xD9 || m == 0x00) return CORRUPT;       // EOI before a scan
        if (pos + 2 > n) return CORRUPT;
        const int len = be16(d + pos);
        if (len < 2 || pos + len > n) return CORRUPT;
        const uint8_t *s = d + pos + 2;
        const int sl = len - 2;
        pos += len;
        if (m == 0xC0 || m == 0xC1) {
            if (sof || sl < 6) return CORRUPT;
            sof = true;
            const int prec = s[0], nc = s[5];
            P.H = be16(s + 1);
            P.W = be16(s + 3);
            if (sl != 6 + 3 * nc) return CORRUPT;
            if (prec != 8 || (nc != 1 && nc != 3)) return UNSUPPORTED;
            if (P.W == 0 || P.H == 0 || P.W > MMR_JPEG_MAX_SIDE || P.H > MMR_JPEG_MAX_SIDE) return UNSUPPORTED;
            P.ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                P.id[c] = s[6 + 3 * c];
                P.h[c] = s[7 + 3 * c] >> 4;
                P.v[c] = s[7 + 3 * c] & 15;
                P.tq[c] = s[8 + 3 * c];
                if (P.h[c] < 1 || P.h[c] > 4 || P.v[c] < 1 || P.v[c] > 4 || P.tq[c] > 3) return CORRUPT;
            }
            if (nc == 1) {
                P.h[0] = P.v[0] = 1;       // one component: its sampling factors mean nothing
            } else {
                if (!sampling_in_scope(3, P.h[0], P.v[0]) || P.h[1] != 1 || P.v[1] != 1 || P.h[2] != 1 || P.v[2] != 1) return UNSUPPORTED;
            }
            P.hmax = P.h[0];
            P.vmax = P.v[0];
            P.mcus_x = mcus_along(P.W, P.hmax);
            P.mcus_y = mcus_along(P.H, P.vmax);
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return UNSUPPORTED;                            // progressive, lossless, arithmetic (SOFn, DAC)
        } else if (m == 0xC4) {
            int at = 0;
            while (at < sl) {
                if (at + 17 > sl) return CORRUPT;
                const int tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 3) return CORRUPT;
                Huff &t = tc ? P.ac[th] : P.dc[th];
                int cnt = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) cnt += (t.bits[l] = s[at + l]);
                t.defined = false;
                if (cnt > 256 || at + 17 + cnt > sl) return CORRUPT;
                memset(t.vals, 0, sizeof(t.vals));
                memcpy(t.vals, s + at + 17, (size_t)cnt);
                if (!huff_derive(t)) return CORRUPT;
                t.defined = true;
                at += 17 + cnt;
            }
        } else if (m == 0xDB) {
            int at = 0;
            while (at < sl) {
                const int pq = s[at] >> 4, tq = s[at] & 15;
                if (tq > 3 || pq > 1) return CORRUPT;
                if (pq == 1) return UNSUPPORTED;           // 16-bit tables
                if (at + 65 > sl) return CORRUPT;
                for (int i = 0; i < 64; ++i) P.qt[tq][kNatural[i]] = s[at + 1 + i];
                P.qt_defined[tq] = true;
                at += 65;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return CORRUPT;
            P.restart = be16(s);
        } else if (m == 0xDC) {
            return UNSUPPORTED;                            // DNL
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!sof || sl < 1) return CORRUPT;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return CORRUPT;
            if (ns != P.ncomp) return UNSUPPORTED;         // one scan per component: several scans
            for (int c = 0; c < ns; ++c) {
                const int cs = s[1 + 2 * c];
                if (cs != P.id[c]) {
                    for (int o = 0; o < P.ncomp; ++o)
                        if (cs == P.id[o]) return UNSUPPORTED;     // a permuted scan
                    return CORRUPT;
                }
                P.td[c] = s[2 + 2 * c] >> 4;
                P.ta[c] = s[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3) return CORRUPT;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return UNSUPPORTED;
            if (P.ncomp == 3) {
                if (adobe && adobe_transform != 1) return UNSUPPORTED;
                if (!jfif && !adobe && P.id[0] == 'R' && P.id[1] == 'G' && P.id[2] == 'B') return UNSUPPORTED;
            }
            for (int c = 0; c < P.ncomp; ++c)
                if (!P.qt_defined[P.tq[c]] || !P.dc[P.td[c]].defined || !P.ac[P.ta[c]].defined) return CORRUPT;
            P.scan = pos;
            return OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

void fill_info(const Parsed &P, int status, mmr_jpeg_info *info)
{
    memset(info, 0, sizeof(*info));
    info->W = P.W;
    info->H = P.H;
    info->status = status;
    if (status != OK) return;
    info->ncomp = P.ncomp;
    info->hmax = P.hmax;
    info->vmax = P.vmax;
    info->mcus_x = P.mcus_x;
    info->mcus_y = P.mcus_y;
    info->blocks0 = (int32_t)component_blocks(P, 0);
    info->blocks1 = (int32_t)component_blocks(P, 1);
    info->blocks2 = (int32_t)component_blocks(P, 2);
    info->coef_bytes = image_blocks(P) * 128;
}

// MSB-first bit reader over one entropy-coded segment.  It stops at a marker (the position stays on its 0xFF) or at the
// end of the data and feeds zero bits from there on; `fake` counts them, and a segment is sound only if none was consumed.
struct Bits {
    const uint8_t *d;
    int64_t pos, end;
    uint64_t buf = 0;
    int n = 0, fake = 0;
    bool stopped = false;

    void fill()
    {
        while (n <= 56) {
            uint64_t b = 0;
            if (!stopped && pos < end) {
                b = d[pos];
                if (b == 0xFF) {
                    if (pos + 1 < end && d[pos + 1] == 0) pos += 2;
                    else { stopped = true; b = 0; }
                } else {
                    ++pos;
                }
            } else {
                stopped = true;
            }
            if (stopped) fake += 8;
            buf = (buf << 8) | b;
            n += 8;
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(buf >> (n - k)) & ((1u << k) - 1u); }
    inline bool sound() const { return n >= fake; }
    void restart() { buf = 0; n = 0; fake = 0; stopped = false; }
};

// one Huffman symbol, -1 for an undefined code
inline int decode_symbol(Bits &b, const Huff &t)
{
    if (b.n < 16) b.fill();
    const uint16_t f = t.fast[b.peek(FAST)];
    if (f) {
        b.n -= f >> 8;
        return f & 255;
    }
    for (int l = FAST + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)b.peek(l);
        if (code <= t.maxcode[l]) {
            const int idx = code + t.delta[l];
            if (idx < 0 || idx > 255) return -1;
            b.n -= l;
            return t.vals[idx];
        }
    }
    return -1;
}

inline int receive_extend(Bits &b, int s)
{
    if (b.n < s) b.fill();
    const int v = (int)b.peek(s);
    b.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int decode_block(Bits &b, const Huff &dc, const Huff &ac, int32_t &pred, int16_t *out)
{
    int s = decode_symbol(b, dc);
    if (s < 0 || s > 15) return CORRUPT;
    if (s) pred += receive_extend(b, s);
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return CORRUPT;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return CORRUPT;
        out[kNatural[k]] = (int16_t)receive_extend(b, s);
        ++k;
    }
    return b.sound() ? OK : CORRUPT;
}

// the marker at `pos` (after fill bytes), -1 for none; leaves pos behind it
int next_marker(const uint8_t *d, int64_t n, int64_t &pos)
{
    if (pos >= n || d[pos] != 0xFF) return -1;
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return -1;
    return d[pos++];
}

int decode_image(const uint8_t *d, int64_t n, const mmr_jpeg_info &info, int16_t *coef, uint16_t *qt)
{
    Parsed P;
    const int st = parse_headers(d, n, P);
    if (st != OK) return st;
    mmr_jpeg_info now;
    fill_info(P, OK, &now);
    if (memcmp(&now, &info, sizeof(now)) != 0) return CORRUPT;     // not the file that was probed
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt[c * 64 + i] = c < P.ncomp ? P.qt[P.tq[c]][i] : 0;
    Bits b{d, P.scan, n};
    int32_t pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)P.mcus_x * P.mcus_y;
    int rst = 0;
    for (int64_t m = 0; m < mcus; ++m) {
        if (P.restart && m && m % P.restart == 0) {
            b.fill();
            if (!b.sound() || b.n - b.fake >= 8) return CORRUPT;
            int64_t pos = b.pos;
            if (next_marker(d, n, pos) != 0xD0 + (rst & 7)) return CORRUPT;
            ++rst;
            b.pos = pos;
            b.restart();
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < P.ncomp; ++c) {
            const int64_t first = blocks_before(P, c), count = component_blocks(P, c);
            int rc = OK;
            mcu_blocks(P, m, c, [&](int64_t blk) {
                rc = blk < 0 || blk >= count ? CORRUPT : decode_block(b, P.dc[P.td[c]], P.ac[P.ta[c]], pred[c], coef + (first + blk) * 64);
                return rc == OK;
            });
            if (rc != OK) return rc;
        }
    }
    b.fill();
    if (!b.sound() || b.n - b.fake >= 8) return CORRUPT;
    int64_t pos = b.pos;
    const int m = next_marker(d, n, pos);
    if (m == 0xD9) return OK;
    if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDC || m == 0xDD || (m >= 0xC0 && m <= 0xCF) || (m >= 0xE0 && m <= 0xFE))
        return UNSUPPORTED;                                // another scan, DNL, or tables for one
    return CORRUPT;
}

}  // namespace

extern "C" {

int mmr_jpeg_probe(const uint8_t *data, int64_t size, mmr_jpeg_info *info)
{
    if (info == nullptr) return MMR_JPEG_CORRUPT;
    Parsed P;
    const int st = (data == nullptr || size < 0) ? CORRUPT : parse_headers(data, size, P);
    fill_info(P, st, info);
    return st;
}

int mmr_jpeg_entropy_decode(const void *datas_host, const int64_t *sizes_host, int B, const mmr_jpeg_info *infos_host,
                            int16_t *coef_host, const int64_t *coef_off_host, uint16_t *qt_host, int32_t *status_host,
                            int threads)
{
    const char *bad = nullptr;
    if (B < 0 || (B > 0 && (!datas_host || !sizes_host || !infos_host || !coef_off_host || !qt_host || !status_host)))
        bad = "mmr_jpeg_entropy_decode: null argument or negative B";
    else if (threads < 1 || threads > 16)
        bad = "mmr_jpeg_entropy_decode: threads must be 1..16";
    for (int i = 0; !bad && i < B; ++i) {
        if (infos_host[i].status == OK && (coef_off_host[i] < 0 || coef_off_host[i] % 16 != 0 || infos_host[i].coef_bytes < 0))
            bad = "mmr_jpeg_entropy_decode: a coefficient offset is negative or no multiple of 16";
        if (infos_host[i].status == OK && infos_host[i].coef_bytes > 0 && !coef_host)
            bad = "mmr_jpeg_entropy_decode: coef_host is null";
    }
    if (bad) return fail(bad);
    const uint8_t *const *datas = (const uint8_t *const *)datas_host;
    parallel_rows(B, threads, [&](int i) {
        uint16_t *qt = qt_host + (size_t)i * 192;
        memset(qt, 0, 192 * sizeof(uint16_t));
        if (infos_host[i].status != OK) {
            status_host[i] = infos_host[i].status;
            return;
        }
        int16_t *coef = (int16_t *)((char *)coef_host + coef_off_host[i]);
        memset(coef, 0, (size_t)infos_host[i].coef_bytes);
        status_host[i] = (datas[i] == nullptr || sizes_host[i] < 0) ? CORRUPT : decode_image(datas[i], sizes_host[i], infos_host[i], coef, qt);
    });
    return MMR_OK;
}

int mmr_jpeg_scan_prepare(const void *datas_host, const int64_t *sizes_host, int B, mmr_jpeg_info *infos_host,
                          mmr_jpeg_scan_desc *scan_desc_host, void *tables_host, uint16_t *qt_host, int32_t *status_host)
{
    if (B < 0 || (B > 0 && (!datas_host || !sizes_host || !infos_host || !scan_desc_host || !tables_host || !qt_host || !status_host)))
        return fail("mmr_jpeg_scan_prepare: null argument or negative B");
    if (((uintptr_t)tables_host & 3) != 0) return fail("mmr_jpeg_scan_prepare: tables_host must be 4-byte aligned");
    const uint8_t *const *datas = (const uint8_t *const *)datas_host;
    int64_t bytes_at = 0, coef_at = 0;
    for (int i = 0; i < B; ++i) {
        mmr_jpeg_scan_desc &D = scan_desc_host[i];
        uint32_t *tables = (uint32_t *)((char *)tables_host + (size_t)i * MMR_JPEG_TABLE_BYTES);
        uint16_t *qt = qt_host + (size_t)i * 192;
        memset(&D, 0, sizeof(D));
        memset(tables, 0, MMR_JPEG_TABLE_BYTES);
        memset(qt, 0, 192 * sizeof(uint16_t));
        Parsed P;
        const int st = (datas[i] == nullptr || sizes_host[i] < 0) ? CORRUPT : parse_headers(datas[i], sizes_host[i], P);
        fill_info(P, st, &infos_host[i]);
        D.status = status_host[i] = st;
        D.tables_off = (int64_t)i * MMR_JPEG_TABLE_BYTES;
        D.bytes_off = D.state_off = bytes_at;
        D.coef_off = coef_at;
        if (st != OK) continue;
        for (int c = 0; c < P.ncomp; ++c)
            for (int k = 0; k < 64; ++k) qt[c * 64 + k] = P.qt[P.tq[c]][k];
        const int64_t scan_bytes = sizes_host[i] - P.scan;
        if (scan_bytes < 2 || scan_bytes > MMR_JPEG_DEVICE_MAX_SCAN) {     // no room for EOI, or longer than the device takes
            D.status = status_host[i] = MMR_JPEG_DECLINED;
            continue;
        }
        // the tables in use, each once: slot = position in `used`; class 0 DC, 1 AC
        int used[6][2], nused = 0, slot[2][3] = {{0, 0, 0}, {0, 0, 0}};
        for (int c = 0; c < P.ncomp; ++c)
            for (int cls = 0; cls < 2; ++cls) {
                const int id = cls ? P.ta[c] : P.td[c];
                int at = 0;
                while (at < nused && !(used[at][0] == cls && used[at][1] == id)) ++at;
                if (at == nused) {
                    used[nused][0] = cls;
                    used[nused][1] = id;
                    ++nused;
                    const Huff &t = cls ? P.ac[id] : P.dc[id];
                    uint32_t *w = tables + (size_t)at * (MMR_JPEG_TABLE_BYTES / 24);      // 6 tables of 336 dwords (jpeg_entropy_core.h)
                    for (int f = 0; f < (1 << FAST); ++f) w[f >> 1] |= (uint32_t)t.fast[f] << (16 * (f & 1));
                    for (int l = FAST + 1; l <= 16; ++l) {
                        w[256 + l - 10] = (uint32_t)t.maxcode[l];
                        w[263 + l - 10] = (uint32_t)t.delta[l];
                    }
                    for (int v = 0; v < 256; ++v) w[270 + (v >> 2)] |= (uint32_t)t.vals[v] << (8 * (v & 3));
                }
                slot[cls][c] = at;
            }
        D.scan_start = P.scan;
        D.scan_bytes = scan_bytes;
        D.restart = P.restart;
        D.ncomp = P.ncomp;
        D.hmax = P.hmax;
        D.vmax = P.vmax;
        D.mcus_x = P.mcus_x;
        D.mcus_y = P.mcus_y;
        D.blocks0 = infos_host[i].blocks0;
        D.blocks1 = infos_host[i].blocks1;
        D.blocks2 = infos_host[i].blocks2;
        D.td0 = slot[0][0]; D.td1 = slot[0][1]; D.td2 = slot[0][2];
        D.ta0 = slot[1][0]; D.ta1 = slot[1][1]; D.ta2 = slot[1][2];
        bytes_at += (scan_bytes + 15) / 16 * 16;
        coef_at += infos_host[i].coef_bytes;
    }
    return MMR_OK;
}

}  // extern "C"
