// The Huffman stage of the JPEG decode as a parallel algorithm: the bit reader, the symbol decode, the decode of one
// subsequence and the DC pass, shared by the device kernel (jpeg_entropy.hip, one lane per call) and by the CPU emulation
// (tests/jpeg_entropy_emul_main.cpp, which runs the same calls lane by lane under the sanitizers).  No HIP call in here.
//
// A scan is cut into subsequences of S raw bytes, counted from its first entropy-coded byte.  The state between two symbols
// is (bit position, block slot within the MCU, zigzag index); `jpe_run<false>` decodes one subsequence from an entry state
// to the first symbol boundary at or past its end and returns the exit state and the blocks it completed, writing nothing.
// The caller repeats rounds of it until no entry state changes; `jpe_run<true>` then decodes each subsequence once more
// under the host stage's rules (jpeg_host.cpp: decode_image / decode_block), with the block ordinal known, and writes the
// coefficients.  The final pass also proves the chain: it starts subsequence 0 in the true state and accepts subsequence k
// only if its exit equals the entry of k + 1, so a row that passes every check has been decoded as one sequential run.
//
// Bounds: a scan byte is read through jpe_word (index checked against the scan's size, zero beyond it), a step consumes at
// least one bit so a subsequence takes at most 8 S + 31 steps, fill bytes before a marker are followed for at most
// JPE_MAX_FILL bytes, and a coefficient is written only behind `offset != JPE_NO_BLOCK` (the block lies inside its
// component's grid) with a zigzag index of at most 63.
//
// The zigzag table (JPEG_NATURAL_ORDER) and the sampling scope are jpeg_geometry.h's.  jpe_geo keeps its own 32-bit block
// counts (the same numbers as component_blocks there; the kernel checks them against the descriptor's).
#pragma once
#include "jpeg_geometry.h"

#define JPE_HD JPEG_HD
#define JPE_NATURAL_ORDER JPEG_NATURAL_ORDER      // the entropy stage's name for the table, kept for its users

namespace mmr_jpe {

constexpr int JPE_FAST = 9;                  // as jpeg_host.cpp's FAST
constexpr int JPE_TABLES = 6;                // table slots per image: at most 3 DC and 3 AC tables are in use
constexpr int JPE_TABLE_WORDS = 336;         // one table: fast[512] u16 | maxcode[10..16] i32 | delta[10..16] i32 | vals[256] u8 (+ pad)
constexpr int JPE_OFF_MAXCODE = 256, JPE_OFF_DELTA = 263, JPE_OFF_VALS = 270;
constexpr uint32_t JPE_END_POS = 0x0FFFFFFFu;   // the bit position of a finished (or abandoned) stream: past every subsequence
constexpr int JPE_LANES = 1024;              // lanes of the workgroup that owns an image (the emulation walks them one by one)
constexpr int JPE_MAX_FILL = 16;             // 0xFF fill bytes followed in front of a marker; more: declined
constexpr uint32_t JPE_NO_BLOCK = 0xFFFFFFFFu;

struct Scan {
    const uint32_t *words;                   // the scan's bytes as little-endian dwords, (nbytes + 3) / 4 of them readable
    uint32_t nbytes;
};

struct Geo {
    int ncomp, hmax, vmax, mcus_x, mcus_y, restart, bpm;      // bpm: blocks per MCU
    uint32_t total, blocks[3], base[3];                       // blocks in all, per component, and each component's first block
    int dc[3], ac[3];                                         // table slot of each component
};

struct Run {
    uint32_t pos;                            // bit position: 8 * (raw byte index) + bits consumed of that byte
    int slot, idx;                           // block slot within the MCU; zigzag index, 0: the DC symbol comes next
    uint32_t blocks;                         // blocks completed by this run
    int bad, done;                           // final pass: a rule of the host stage failed; EOI found behind the last block
};

JPE_HD bool jpe_geo(Geo &G, int ncomp, int hmax, int vmax, int mcus_x, int mcus_y, int restart, const int *dc, const int *ac)
{
    if (!mmr_jpeg::sampling_in_scope(ncomp, hmax, vmax) || mcus_x < 1 || mcus_y < 1 || mcus_x > 2048 || mcus_y > 2048 || restart < 0 || restart > 65535) return false;
    G.ncomp = ncomp; G.hmax = hmax; G.vmax = vmax; G.mcus_x = mcus_x; G.mcus_y = mcus_y; G.restart = restart;
    const uint32_t mcus = (uint32_t)mcus_x * (uint32_t)mcus_y;
    G.bpm = ncomp == 1 ? 1 : hmax * vmax + 2;
    G.blocks[0] = mcus * (uint32_t)(hmax * vmax);
    G.blocks[1] = G.blocks[2] = ncomp == 3 ? mcus : 0;
    G.base[0] = 0; G.base[1] = G.blocks[0]; G.base[2] = G.blocks[0] + G.blocks[1];
    G.total = G.blocks[0] + G.blocks[1] + G.blocks[2];
    for (int c = 0; c < 3; ++c) {
        G.dc[c] = dc[c]; G.ac[c] = ac[c];
        if (dc[c] < 0 || dc[c] >= JPE_TABLES || ac[c] < 0 || ac[c] >= JPE_TABLES) return false;
    }
    return true;
}

JPE_HD uint32_t jpe_word(const Scan &s, uint32_t wi) { return wi < ((s.nbytes + 3u) >> 2) ? s.words[wi] : 0u; }
JPE_HD uint32_t jpe_byte(const Scan &s, uint32_t at) { return at < s.nbytes ? (jpe_word(s, at >> 2) >> (8 * (at & 3))) & 255u : 0u; }

// The next 32 bits from (byte p, bit b), MSB first, as jpeg_host.cpp's Bits feeds them: FF 00 is one data byte, a marker
// or the end of the data stops the reader and zero bits follow.  `real` counts the bits in front of the stop.
struct Win {
    uint32_t bits, stuffed, stop_at;         // stuffed: bit i set when data byte i of the window was an FF 00 pair
    int real, stop;                          // stop: 0 none within the window, 1 a marker's FF at stop_at, 2 the end of the data
};

JPE_HD void jpe_window(const Scan &s, uint32_t p, int b, Win &w)
{
    const uint32_t wi = p >> 2;
    const uint64_t lo = (uint64_t)jpe_word(s, wi) | ((uint64_t)jpe_word(s, wi + 1) << 32);
    const uint64_t hi = (uint64_t)jpe_word(s, wi + 2) | ((uint64_t)jpe_word(s, wi + 3) << 32);
    int o = (int)(p & 3);                    // at most 3 + 5 * 2 + 1 = 14 < 16
    uint32_t q = p;
    uint64_t acc = 0;
    int real = 0;
    w.stuffed = 0; w.stop = 0; w.stop_at = 0;
    for (int i = 0; i < 5; ++i) {
        uint32_t c = 0;
        if (!w.stop) {
            if (q >= s.nbytes) {
                w.stop = 2; w.stop_at = q;
            } else {
                c = (uint32_t)((o < 8 ? lo >> (8 * o) : hi >> (8 * (o - 8))) & 255u);
                if (c == 0xFF) {
                    const int o1 = o + 1;
                    const uint32_t c1 = q + 1 < s.nbytes ? (uint32_t)((o1 < 8 ? lo >> (8 * o1) : hi >> (8 * (o1 - 8))) & 255u) : 1u;
                    if (c1 == 0) { w.stuffed |= 1u << i; q += 2; o += 2; }
                    else { w.stop = 1; w.stop_at = q; c = 0; }
                } else {
                    ++q; ++o;
                }
                if (!w.stop) real += 8;
            }
        }
        acc = (acc << 8) | c;
    }
    w.bits = (uint32_t)((acc << b) >> 8);
    w.real = real > b ? real - b : 0;
}

// (p, b) moved on by n <= real bits of the window built at (p, b)
JPE_HD uint32_t jpe_advance(const Win &w, uint32_t p, int b, int n)
{
    const int nb = (b + n) >> 3;             // at most (7 + 31) / 8 = 4 data bytes
    uint32_t m = w.stuffed & ((1u << nb) - 1u), extra = 0;
    for (; m; m &= m - 1) ++extra;
    return ((p + (uint32_t)nb + extra) << 3) | (uint32_t)((b + n) & 7);
}

// the marker code behind the FF at `at` and its fill bytes, -1 for none (or too many fill bytes); after: the byte behind it
JPE_HD int jpe_marker(const Scan &s, uint32_t at, uint32_t &after)
{
    uint32_t q = at;
    int n = 0;
    while (n <= JPE_MAX_FILL && q < s.nbytes && jpe_byte(s, q) == 0xFF) { ++q; ++n; }
    if (n == 0 || n > JPE_MAX_FILL || q >= s.nbytes) return -1;
    after = q + 1;
    return (int)jpe_byte(s, q);
}

JPE_HD int jpe_comp_of_slot(const Geo &G, int slot)
{
    const int hv = G.hmax * G.vmax;
    return G.ncomp == 1 || slot < hv ? 0 : (slot == hv ? 1 : 2);
}

// scan-order block ordinal -> the int16 offset of its 64 coefficients (decode_image's map), JPE_NO_BLOCK outside the grids
JPE_HD uint32_t jpe_block_offset(const Geo &G, uint32_t g)
{
    if (g >= G.total) return JPE_NO_BLOCK;
    const uint32_t m = g / (uint32_t)G.bpm;
    const int slot = (int)(g - m * (uint32_t)G.bpm);
    const int c = jpe_comp_of_slot(G, slot);
    const uint32_t h = c == 0 ? (uint32_t)G.hmax : 1u, v = c == 0 ? (uint32_t)G.vmax : 1u;
    const uint32_t in = c == 0 ? (uint32_t)slot : 0u, by = in / h, bx = in - by * h;
    const uint32_t my = m / (uint32_t)G.mcus_x, mx = m - my * (uint32_t)G.mcus_x;
    const uint32_t blk = (my * v + by) * ((uint32_t)G.mcus_x * h) + mx * h + bx;
    if (by >= v || blk >= G.blocks[c]) return JPE_NO_BLOCK;
    return (G.base[c] + blk) * 64u;
}

// where subsequence k > 0 starts when nothing is known: its first byte, or the byte behind it if that one is the 00 of an FF 00
JPE_HD uint32_t jpe_default_pos(const Scan &s, uint32_t k, uint32_t S)
{
    const uint32_t p = k * S;
    return (p > 0 && jpe_byte(s, p - 1) == 0xFF && p < s.nbytes && jpe_byte(s, p) == 0 ? p + 1 : p) << 3;
}

// whether fewer than 8 bits stand between `pos` and a marker or the end of the data; m: the marker's code, -1 for none
JPE_HD bool jpe_boundary(const Scan &s, uint32_t pos, int &m, uint32_t &after)
{
    Win w;
    jpe_window(s, pos >> 3, (int)(pos & 7), w);
    m = -1;
    if (!(w.real < 8 && w.stop)) return false;
    if (w.stop == 1) m = jpe_marker(s, w.stop_at, after);
    return true;
}

// One subsequence: from the state in `r` to the first symbol boundary at or past end_bits.
// FINAL = false (a round): never fails.  An undefined code costs one bit, an index past 63 ends the block; at an MCU
// boundary with fewer than 8 bits in front of a marker, and wherever a symbol would need bits past a marker, RSTn puts the
// lane into the state behind it (slot 0, index 0) and anything else ends the stream (JPE_END_POS).
// FINAL = true: `g` is the ordinal of the block the entry state is in.  The host stage's rules apply; a failure sets r.bad
// and ends the stream.  DC differences are written to coefficient 0 (jpe_dc_range sums them afterwards).
template <bool FINAL>
JPE_HD void jpe_run(const Scan &s, const uint32_t *tables, const Geo &G, const uint8_t *natural, uint32_t end_bits, int max_steps,
                    Run &r, uint32_t g, int16_t *coef)
{
    r.blocks = 0; r.bad = 0; r.done = 0;
    uint32_t off = JPE_NO_BLOCK;
    if (FINAL) {
        if (r.pos < end_bits && (uint32_t)r.slot != g % (uint32_t)G.bpm) { r.bad = 1; r.pos = JPE_END_POS; return; }
        off = jpe_block_offset(G, g);
    }
    const uint32_t per_restart = (uint32_t)G.restart * (uint32_t)G.bpm;
    for (int step = 0; r.pos < end_bits; ++step) {
        if (step >= max_steps) { r.bad = 1; r.pos = JPE_END_POS; break; }
        const uint32_t p = r.pos >> 3;
        const int b = (int)(r.pos & 7);
        Win w;
        jpe_window(s, p, b, w);
        uint32_t after = 0;
        if (!FINAL && r.idx == 0 && r.slot == 0 && w.real < 8 && w.stop) {      // a guessed state in front of a marker
            const int m = w.stop == 1 ? jpe_marker(s, w.stop_at, after) : -1;
            if (m >= 0xD0 && m <= 0xD7) { r.pos = after << 3; continue; }
            r.pos = JPE_END_POS;
            break;
        }
        const int c = jpe_comp_of_slot(G, r.slot);
        const uint32_t *T = tables + JPE_TABLE_WORDS * (r.idx == 0 ? G.dc[c] : G.ac[c]);
        int len = 0, sym = -1;
        const uint32_t fi = w.bits >> (32 - JPE_FAST);
        const uint32_t f = (T[fi >> 1] >> (16 * (fi & 1))) & 0xFFFFu;
        if (f) {
            len = (int)(f >> 8); sym = (int)(f & 255);
        } else {
            for (int l = JPE_FAST + 1; l <= 16; ++l) {
                const int32_t code = (int32_t)(w.bits >> (32 - l));
                if (code <= (int32_t)T[JPE_OFF_MAXCODE + l - 10]) {
                    const int32_t i = code + (int32_t)T[JPE_OFF_DELTA + l - 10];
                    if (i >= 0 && i <= 255) { len = l; sym = (int)((T[JPE_OFF_VALS + (i >> 2)] >> (8 * (i & 3))) & 255u); }
                    break;
                }
            }
        }
        int ext = 0, next = 0, k = 0;
        bool wrong = sym < 0 || len < 1 || len > 16, write = false;
        if (!wrong) {
            if (r.idx == 0) {
                if (sym > 15) wrong = true;
                else { ext = sym; next = 1; write = true; }
            } else if ((sym & 15) == 0) {
                next = (sym >> 4) == 15 ? r.idx + 16 : 64;                  // ZRL, or end of block
            } else {
                ext = sym & 15;
                k = r.idx + (sym >> 4);
                next = k + 1;
                if (k > 63) { if (FINAL) wrong = true; else { next = 64; } }
                else write = true;
            }
        }
        if (wrong) {
            if (FINAL) { r.bad = 1; r.pos = JPE_END_POS; break; }
            len = 1; ext = 0; next = r.idx; write = false;                  // resynchronise: drop one bit, keep the state
        }
        const int n = len + ext;                                            // at most 16 + 15
        if (n > w.real) {                                                   // the symbol needs bits that are not there
            if (FINAL) { r.bad = 1; r.pos = JPE_END_POS; break; }
            const int m = w.stop == 1 ? jpe_marker(s, w.stop_at, after) : -1;
            if (m >= 0xD0 && m <= 0xD7) { r.pos = after << 3; r.slot = 0; r.idx = 0; continue; }
            r.pos = JPE_END_POS; r.slot = 0; r.idx = 0;
            break;
        }
        if (FINAL && write) {
            int v = 0;
            if (ext) {
                v = (int)((w.bits << len) >> (32 - ext));
                if (v < (1 << (ext - 1))) v += 1 - (1 << ext);
            }
            if (off != JPE_NO_BLOCK && k >= 0 && k <= 63) coef[off + natural[k]] = (int16_t)v;
            else { r.bad = 1; r.pos = JPE_END_POS; break; }
        }
        r.pos = jpe_advance(w, p, b, n);
        if (next >= 64) {
            r.idx = 0;
            r.slot = r.slot + 1 >= G.bpm ? 0 : r.slot + 1;
            ++r.blocks;
            if (FINAL) { ++g; off = jpe_block_offset(G, g); }
            // behind an MCU: the restart marker or EOI, as decode_image looks for them.  The final pass knows when one is
            // due; a round takes fewer than 8 bits in front of a marker for the sign.
            const bool last = FINAL && g == G.total, due = FINAL && !last && per_restart && g % per_restart == 0;
            if (FINAL ? (last || due) : r.slot == 0) {
                int m = -1;
                const bool at_marker = jpe_boundary(s, r.pos, m, after);
                if (FINAL) {
                    if (last) {
                        if (at_marker && m == 0xD9) r.done = 1;
                        else r.bad = 1;
                        r.pos = JPE_END_POS;
                        break;
                    }
                    if (!(at_marker && m == 0xD0 + (int)((g / per_restart - 1) & 7))) { r.bad = 1; r.pos = JPE_END_POS; break; }
                    r.pos = after << 3;
                } else if (at_marker) {
                    if (m >= 0xD0 && m <= 0xD7) r.pos = after << 3;
                    else { r.pos = JPE_END_POS; break; }
                }
            }
        } else {
            r.idx = next;
        }
    }
}

// The DC pass over MCUs [m0, m1) of component c, after the final pass left DC differences in coefficient 0: the running
// sum modulo 2^16 (decode_block keeps int32 and stores the low 16 bits), zero at every restart interval.  apply = false
// only sums: `sum` is the sum behind the last reset of the range (or over all of it), `reset` whether there was one.
JPE_HD void jpe_dc_range(const Geo &G, int c, uint32_t m0, uint32_t m1, int16_t *coef, bool apply, uint32_t &sum, int &reset)
{
    const uint32_t h = c == 0 ? (uint32_t)G.hmax : 1u, v = c == 0 ? (uint32_t)G.vmax : 1u, bw = (uint32_t)G.mcus_x * h;
    for (uint32_t m = m0; m < m1; ++m) {
        if (G.restart && m % (uint32_t)G.restart == 0) { sum = 0; reset = 1; }
        const uint32_t my = m / (uint32_t)G.mcus_x, mx = m - my * (uint32_t)G.mcus_x;
        for (uint32_t by = 0; by < v; ++by)
            for (uint32_t bx = 0; bx < h; ++bx) {
                const uint32_t blk = (my * v + by) * bw + mx * h + bx;
                if (blk >= G.blocks[c]) continue;
                int16_t *e = coef + (size_t)(G.base[c] + blk) * 64u;
                sum = (sum + (uint32_t)(uint16_t)*e) & 0xFFFFu;
                if (apply) *e = (int16_t)(uint16_t)sum;
            }
    }
}

}  // namespace mmr_jpe
