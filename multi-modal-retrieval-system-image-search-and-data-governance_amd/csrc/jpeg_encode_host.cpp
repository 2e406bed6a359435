// Host stage of the JPEG encode: libjpeg's quality scaling of the Annex K quantisation tables, the Huffman (entropy) coder
// with the Annex K tables on up to 16 std::threads, and the file framing.  Plain C++17 with no HIP call: it also builds
// with g++ (tests/jpeg_encode_main.cpp runs it under the address and undefined-behaviour sanitizers).  The device stage
// is jpeg_encode.hip; the contract of both is in mmr.h, the arithmetic in DESIGN.md section "JPEG encode".  The block
// layout and the order of a scan are jpeg_geometry.h's; error reporting and the thread pool jpeg_host_util.h's.
//
// Every byte goes out through Writer::put, which compares the position with the capacity the caller passed; every
// coefficient read stays inside the block counts the geometry gives.
#include <string.h>

#include "jpeg_host_util.h"

namespace {

using namespace mmr_jpeg;

const uint8_t kNatural[64] = JPEG_NATURAL_ORDER;

// ITU-T T.81 Annex K.1, natural order
const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                              69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                              81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// ITU-T T.81 Annex K.3: code counts per length 1..16, then the symbols
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int OK = MMR_JPEG_OK, UNSUPPORTED = MMR_JPEG_UNSUPPORTED, NO_ROOM = MMR_JPEG_NO_ROOM;
constexpr int64_t HEADER_BOUND = 1024;      // the segments before and after the scan take 623 bytes at most

// symbol -> (code, length); length 0: the table has no such symbol
struct Codes {
    uint16_t code[256];
    uint8_t size[256];
    const uint8_t *bits, *vals;
    int count;
};

void derive(Codes &t, const uint8_t *bits, const uint8_t *vals)
{
    memset(t.code, 0, sizeof(t.code));
    memset(t.size, 0, sizeof(t.size));
    t.bits = bits;
    t.vals = vals;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            t.code[vals[k]] = (uint16_t)code;
            t.size[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
    t.count = k;
}

struct Tables {
    Codes dc[2], ac[2];
    Tables()
    {
        derive(dc[0], kDcLumaBits, kDcVals);
        derive(dc[1], kDcChromaBits, kDcVals);
        derive(ac[0], kAcLumaBits, kAcLumaVals);
        derive(ac[1], kAcChromaBits, kAcChromaVals);
    }
};

// Bytes and MSB-first bits into [out, out + cap).  A byte that does not fit is dropped and remembered.
struct Writer {
    uint8_t *out;
    int64_t cap, pos = 0;
    uint64_t acc = 0;
    int n = 0;                 // bits waiting in acc (fewer than 8 between calls of bits())
    bool full = false;

    inline void put(int b)
    {
        if (pos < cap) out[pos++] = (uint8_t)b;
        else full = true;
    }
    inline void put16(int v) { put(v >> 8); put(v & 255); }
    void bytes(const uint8_t *p, int count) { for (int i = 0; i < count; ++i) put(p[i]); }
    // entropy-coded bits: a 00 follows every FF
    inline void bits(uint32_t v, int len)
    {
        acc = (acc << len) | (v & ((1u << len) - 1u));
        n += len;
        while (n >= 8) {
            const int b = (int)(acc >> (n - 8)) & 255;
            put(b);
            if (b == 255) put(0);
            n -= 8;
        }
    }
    inline void pad()          // fill the last byte with 1-bits
    {
        if (n) bits(0x7f, 8 - n);
        acc = 0;
        n = 0;
    }
};

inline int bit_length(unsigned v)
{
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

// one block; false for a value the baseline tables cannot code
inline bool encode_block(Writer &w, const Codes &dc, const Codes &ac, int &pred, const int16_t *blk)
{
    const int diff = (int)blk[0] - pred;
    pred = blk[0];
    int s = bit_length((unsigned)(diff < 0 ? -diff : diff));
    if (s > 11) return false;
    w.bits(dc.code[s], dc.size[s]);
    if (s) w.bits((unsigned)(diff < 0 ? diff - 1 : diff), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[kNatural[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) w.bits(ac.code[0xF0], ac.size[0xF0]);
        s = bit_length((unsigned)(v < 0 ? -v : v));
        if (s > 10) return false;
        const int sym = (run << 4) | s;
        w.bits(ac.code[sym], ac.size[sym]);
        w.bits((unsigned)(v < 0 ? v - 1 : v), s);
        run = 0;
    }
    if (run) w.bits(ac.code[0], ac.size[0]);
    return true;
}

bool in_scope(const mmr_jpeg_info &f)
{
    if (f.status != OK || !sampling_in_scope(f.ncomp, f.hmax, f.vmax) || !grid_in_scope(f, MMR_JPEG_MAX_SIDE)) return false;
    return f.blocks0 == component_blocks(f, 0) && f.blocks1 == component_blocks(f, 1) && f.blocks2 == component_blocks(f, 2) &&
           f.coef_bytes == image_blocks(f) * 128;
}

void write_dht(Writer &w, int id, const Codes &t)
{
    w.put16(0xFFC4);
    w.put16(2 + 1 + 16 + t.count);
    w.put(id);
    w.bytes(t.bits, 16);
    w.bytes(t.vals, t.count);
}

int encode_image(const Tables &T, const mmr_jpeg_info &f, const int16_t *coef, const uint16_t *qt, int restart, Writer &w)
{
    if (!in_scope(f)) return UNSUPPORTED;
    const int nc = f.ncomp, ntab = nc == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t)
        for (int i = 0; i < 64; ++i)
            if (qt[t * 64 + i] < 1 || qt[t * 64 + i] > 255) return UNSUPPORTED;
    static const uint8_t app0[18] = {0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    w.put16(0xFFD8);
    w.bytes(app0, 18);
    for (int t = 0; t < ntab; ++t) {
        w.put16(0xFFDB);
        w.put16(0x43);
        w.put(t);
        for (int i = 0; i < 64; ++i) w.put(qt[t * 64 + kNatural[i]]);
    }
    w.put16(0xFFC0);
    w.put16(8 + 3 * nc);
    w.put(8);
    w.put16(f.H);
    w.put16(f.W);
    w.put(nc);
    for (int c = 0; c < nc; ++c) {
        w.put(c + 1);
        w.put(c == 0 ? ((f.hmax << 4) | f.vmax) : 0x11);
        w.put(c == 0 ? 0 : 1);
    }
    write_dht(w, 0x00, T.dc[0]);
    write_dht(w, 0x10, T.ac[0]);
    if (nc == 3) {
        write_dht(w, 0x01, T.dc[1]);
        write_dht(w, 0x11, T.ac[1]);
    }
    if (restart > 0) {
        w.put16(0xFFDD);
        w.put16(4);
        w.put16(restart);
    }
    w.put16(0xFFDA);
    w.put16(6 + 2 * nc);
    w.put(nc);
    for (int c = 0; c < nc; ++c) {
        w.put(c + 1);
        w.put(c == 0 ? 0x00 : 0x11);
    }
    w.put(0);
    w.put(63);
    w.put(0);

    int pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;
    int rst = 0;
    for (int64_t m = 0; m < mcus && !w.full; ++m) {
        if (restart > 0 && m && m % restart == 0) {
            w.pad();
            w.put16(0xFFD0 + (rst & 7));
            ++rst;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < nc; ++c) {
            const int16_t *first = coef + blocks_before(f, c) * 64;
            if (!mcu_blocks(f, m, c, [&](int64_t blk) { return encode_block(w, T.dc[c ? 1 : 0], T.ac[c ? 1 : 0], pred[c], first + blk * 64); }))
                return UNSUPPORTED;
        }
    }
    w.pad();
    w.put16(0xFFD9);
    return w.full ? NO_ROOM : OK;
}

}  // namespace

extern "C" {

int mmr_jpeg_quant_tables(int quality, uint16_t *qt_luma, uint16_t *qt_chroma)
{
    if (quality < 1 || quality > 100 || !qt_luma || !qt_chroma) {
        if (mmr::set_error) mmr::set_error("mmr_jpeg_quant_tables: quality=%d outside 1..100, or a null table", quality);
        return MMR_EINVAL;
    }
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (kStdLuma[i] * s + 50) / 100, c = (kStdChroma[i] * s + 50) / 100;
        qt_luma[i] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        qt_chroma[i] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    return MMR_OK;
}

int64_t mmr_jpeg_encode_bound(const mmr_jpeg_info *info)
{
    if (!info || !in_scope(*info)) return 0;
    // a block: at most 11 + 11 bits of DC and 63 x (16 + 10) bits of AC, 208 bytes, each possibly followed by a stuffed
    // zero; an MCU: a restart marker and one padded, stuffed byte in front of it
    return HEADER_BOUND + image_blocks(*info) * 416 + (int64_t)info->mcus_x * info->mcus_y * 4;
}

int mmr_jpeg_entropy_encode(const int16_t *coef_host, const int64_t *coef_off_host, const mmr_jpeg_info *infos_host,
                            const uint16_t *qt_host, int B, int restart_interval, uint8_t *out_host,
                            const int64_t *out_off_host, const int64_t *out_cap_host, int64_t *out_bytes_host,
                            int32_t *status_host, int threads)
{
    const char *bad = nullptr;
    if (B < 0 || (B > 0 && (!coef_host || !coef_off_host || !infos_host || !qt_host || !out_off_host || !out_cap_host || !out_bytes_host || !status_host)))
        bad = "mmr_jpeg_entropy_encode: null argument or negative B";
    else if (threads < 1 || threads > 16)
        bad = "mmr_jpeg_entropy_encode: threads must be 1..16";
    else if (restart_interval < 0 || restart_interval > 65535)
        bad = "mmr_jpeg_entropy_encode: restart_interval must be 0..65535";
    for (int i = 0; !bad && i < B; ++i) {
        if (coef_off_host[i] < 0 || coef_off_host[i] % 2 != 0) bad = "mmr_jpeg_entropy_encode: a coefficient offset is negative or odd";
        else if (out_off_host[i] < 0 || out_cap_host[i] < 0) bad = "mmr_jpeg_entropy_encode: a negative output offset or capacity";
        else if (out_cap_host[i] > 0 && !out_host) bad = "mmr_jpeg_entropy_encode: out_host is null";
    }
    if (bad) return fail(bad);
    const Tables T;
    parallel_rows(B, threads, [&](int i) {
        Writer w{out_cap_host[i] > 0 ? out_host + out_off_host[i] : nullptr, out_cap_host[i]};
        const int st = encode_image(T, infos_host[i], (const int16_t *)((const char *)coef_host + coef_off_host[i]), qt_host + (size_t)i * 192,
                                    restart_interval, w);
        status_host[i] = st;
        out_bytes_host[i] = st == OK ? w.pos : 0;
    });
    return MMR_OK;
}

}  // extern "C"
