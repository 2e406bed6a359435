// CPU emulation of the device Huffman stage (csrc/jpeg_entropy.hip) through the header both share
// (csrc/jpeg_entropy_core.h), for a sanitizer build: tests/test_jpeg_entropy_host.py compiles this file and
// csrc/jpeg_host.cpp with g++ -fsanitize=address,undefined and runs the result as a child process:
//     jpeg_entropy_emul --subseq S... [--good FILE...] [--pack PACKFILE...]
// Every file runs through mmr_jpeg_scan_prepare and then through the kernel's steps, lane by lane in the kernel's order
// (JPE_LANES lanes, subsequence k on lane k % JPE_LANES): rounds until no entry state changes, the prefix sum, the final pass, the DC
// pass.  Scan bytes, states and coefficients live in heap blocks of exactly the sizes the kernel may touch, so a read or a
// write outside them is a sanitizer report.  The result is compared with the host stage, mmr_jpeg_entropy_decode:
//   --good   the file must come out with status 0 on both sides and equal coefficients, at max_rounds = 1024
//   --pack   a file of records (uint32 length, bytes): mutated files, at max_rounds = number of subsequences; status 0 on
//            one side if and only if on the other, equal coefficients where 0
// Prints `rounds NAME S=.. rounds=.. subseq=..` per good file and a summary; exit status 0 if everything held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/mmr.h"
#include "jpeg_entropy_core.h"

using namespace mmr_jpe;

static const int LANES = JPE_LANES;
static const uint32_t DIRTY = 0x80000000u;

struct Result {
    int status = MMR_JPEG_DECLINED, rounds = 0;
    uint32_t nsub = 0;
};

static uint32_t aux_of(const Run &r) { return (uint32_t)r.idx | ((uint32_t)r.slot << 6); }

// the kernel, one image; `coef` has exactly the image's span
static Result emulate(const mmr_jpeg_scan_desc &d, const uint8_t *file, const uint32_t *tables, int16_t *coef, int S, int max_rounds)
{
    static const uint8_t natural[64] = JPE_NATURAL_ORDER;
    Result out;
    Geo G;
    const int dcs[3] = {d.td0, d.td1, d.td2}, acs[3] = {d.ta0, d.ta1, d.ta2};
    if (d.status != 0 || d.ncomp == 0) {
        out.status = d.status ? d.status : MMR_JPEG_DECLINED;
        return out;
    }
    if (!jpe_geo(G, d.ncomp, d.hmax, d.vmax, d.mcus_x, d.mcus_y, d.restart, dcs, acs)) return out;
    const uint32_t nbytes = (uint32_t)d.scan_bytes, nsub = (nbytes + S - 1) / S;
    out.nsub = nsub;
    const size_t nwords = (nbytes + 3u) / 4u;
    uint32_t *words = (uint32_t *)malloc(nwords * 4);
    memset(words, 0xEE, nwords * 4);                      // the bytes behind the scan's end inside the last dword are never data
    memcpy(words, file + d.scan_start, nbytes);
    const Scan scan = {words, nbytes};
    uint32_t *e_pos = (uint32_t *)malloc(4 * (size_t)nsub), *e_aux = (uint32_t *)malloc(4 * (size_t)nsub);
    uint32_t *x_pos = (uint32_t *)malloc(4 * (size_t)nsub), *x_aux = (uint32_t *)malloc(4 * (size_t)nsub);
    memset(coef, 0, (size_t)G.total * 128);
    for (uint32_t k = 0; k < nsub; ++k) {
        e_pos[k] = k ? jpe_default_pos(scan, k, (uint32_t)S) : 0u;
        e_aux[k] = DIRTY;
    }
    const int max_steps = 8 * S + 31;
    auto end_of = [&](uint32_t k) { return (k + 1u) * (uint32_t)S < nbytes ? (k + 1u) * (uint32_t)S * 8u : nbytes * 8u; };
    bool converged = false;
    while (out.rounds < max_rounds && !converged) {
        ++out.rounds;
        bool changed = false;
        for (int tid = 0; tid < LANES; ++tid)
            for (uint32_t k = tid; k < nsub; k += LANES) {
                const uint32_t aux = e_aux[k];
                if (!(aux & DIRTY)) continue;
                Run r;
                r.pos = e_pos[k]; r.idx = (int)(aux & 63u); r.slot = (int)((aux >> 6) & 7u);
                jpe_run<false>(scan, tables, G, natural, end_of(k), max_steps, r, 0u, nullptr);
                x_pos[k] = r.pos;
                x_aux[k] = aux_of(r) | (r.blocks << 16);
                e_aux[k] = aux & ~DIRTY;
            }
        for (int tid = 0; tid < LANES; ++tid)
            for (uint32_t k = tid; k + 1u < nsub; k += LANES) {
                const uint32_t xp = x_pos[k], xa = x_aux[k] & 0x1FFu;
                if (xp != e_pos[k + 1] || xa != (e_aux[k + 1] & 0x1FFu)) {
                    e_pos[k + 1] = xp;
                    e_aux[k + 1] = xa | DIRTY;
                    changed = true;
                }
            }
        converged = !changed;
    }
    int bad = 0, done = 0;
    if (converged) {
        uint32_t g = 0;
        for (uint32_t k = 0; k < nsub; ++k) {
            x_pos[k] = g;
            g += x_aux[k] >> 16;
        }
        for (int tid = 0; tid < LANES; ++tid)
            for (uint32_t k = tid; k < nsub; k += LANES) {
                const uint32_t aux = e_aux[k], g0 = x_pos[k];
                Run r;
                r.pos = e_pos[k]; r.idx = (int)(aux & 63u); r.slot = (int)((aux >> 6) & 7u);
                jpe_run<true>(scan, tables, G, natural, end_of(k), max_steps, r, g0, coef);
                bad |= r.bad;
                done += r.done;
                if (!r.bad && k + 1u < nsub && (r.pos != e_pos[k + 1] || aux_of(r) != (e_aux[k + 1] & 0x1FFu) || g0 + r.blocks != x_pos[k + 1])) bad = 1;
            }
    }
    const bool good = converged && !bad && done == 1;
    if (good) {
        const uint32_t mcus = (uint32_t)G.mcus_x * (uint32_t)G.mcus_y, per = (mcus + LANES - 1u) / LANES;
        std::vector<uint32_t> sums(3 * LANES);
        std::vector<int> resets(3 * LANES);
        auto lo = [&](int tid) { return (uint32_t)tid * per < mcus ? (uint32_t)tid * per : mcus; };
        for (int tid = 0; tid < LANES; ++tid)
            for (int c = 0; c < G.ncomp; ++c) {
                uint32_t sum = 0;
                int reset = 0;
                jpe_dc_range(G, c, lo(tid), lo(tid + 1), coef, false, sum, reset);
                sums[c * LANES + tid] = sum;
                resets[c * LANES + tid] = reset;
            }
        for (int tid = 0; tid < LANES; ++tid)
            for (int c = 0; c < G.ncomp; ++c) {
                uint32_t sum = 0;
                for (int j = 0; j < tid; ++j) sum = resets[c * LANES + j] ? sums[c * LANES + j] : (sum + sums[c * LANES + j]) & 0xFFFFu;
                int reset = 0;
                jpe_dc_range(G, c, lo(tid), lo(tid + 1), coef, true, sum, reset);
            }
    }
    free(words); free(e_pos); free(e_aux); free(x_pos); free(x_aux);
    out.status = good ? MMR_JPEG_OK : MMR_JPEG_DECLINED;
    return out;
}

static long n_good, n_mut, n_accepted, n_declined, failures;

// one file, at subsequence size S; must_decode: a --good file
static void check(const std::vector<uint8_t> &file, const std::string &name, int S, bool must_decode)
{
    uint8_t *data = (uint8_t *)malloc(file.size() ? file.size() : 1);
    if (!file.empty()) memcpy(data, file.data(), file.size());
    const void *datas[1] = {data};
    const int64_t sizes[1] = {(int64_t)file.size()};
    mmr_jpeg_info info;
    mmr_jpeg_scan_desc desc;
    uint32_t *tables = (uint32_t *)malloc(MMR_JPEG_TABLE_BYTES);
    uint16_t qt[192], qt_host[192];
    int32_t status = -1, host_status = -1;
    if (mmr_jpeg_scan_prepare(datas, sizes, 1, &info, &desc, tables, qt, &status) != MMR_OK) {
        fprintf(stderr, "%s: mmr_jpeg_scan_prepare rejected its arguments\n", name.c_str());
        exit(2);
    }
    mmr_jpeg_info probed;
    mmr_jpeg_probe(data, (int64_t)file.size(), &probed);
    if (memcmp(&probed, &info, sizeof(info)) != 0 || (status != probed.status && status != MMR_JPEG_DECLINED)) {
        fprintf(stderr, "%s: the prepared info or status is not the probe's\n", name.c_str());
        ++failures;
    }
    if (probed.status == MMR_JPEG_OK) {
        const size_t n = (size_t)info.coef_bytes / 2;
        int16_t *want = (int16_t *)aligned_alloc(16, (info.coef_bytes + 15) / 16 * 16), *got = (int16_t *)malloc(n * 2 ? n * 2 : 1);
        const int64_t off[1] = {0};
        mmr_jpeg_entropy_decode(datas, sizes, 1, &probed, want, off, qt_host, &host_status, 1);
        Result r;
        if (status == MMR_JPEG_OK) {
            const uint32_t nsub = (uint32_t)((desc.scan_bytes + S - 1) / S);
            r = emulate(desc, data, tables, got, S, must_decode ? 1024 : (int)(nsub < 1 ? 1 : (nsub > 1024 ? 1024 : nsub)));
        }
        const bool same = r.status == MMR_JPEG_OK && memcmp(got, want, n * 2) == 0 && memcmp(qt, qt_host, sizeof(qt)) == 0;
        if (must_decode) {
            printf("rounds %s S=%d rounds=%d subseq=%u\n", name.c_str(), S, r.rounds, r.nsub);
            if (host_status != MMR_JPEG_OK || !same) {
                fprintf(stderr, "%s S=%d: host status %d, emulated status %d, coefficients %s\n", name.c_str(), S, host_status, r.status, same ? "equal" : "differ");
                ++failures;
            }
            ++n_good;
        } else {
            ++n_mut;
            if (r.status == MMR_JPEG_OK) ++n_accepted; else ++n_declined;
            if ((r.status == MMR_JPEG_OK) != (host_status == MMR_JPEG_OK) || (r.status == MMR_JPEG_OK && !same)) {
                fprintf(stderr, "%s S=%d: host status %d, emulated status %d after %d rounds of %u subsequences, coefficients %s\n", name.c_str(), S,
                        host_status, r.status, r.rounds, r.nsub, same ? "equal" : "differ");
                ++failures;
            }
        }
        free(want);
        free(got);
    } else if (must_decode) {
        fprintf(stderr, "%s: probe status %d\n", name.c_str(), probed.status);
        ++failures;
    } else {
        ++n_mut;
        ++n_declined;
    }
    free(tables);
    free(data);
}

static std::vector<uint8_t> slurp(const char *name)
{
    FILE *fh = fopen(name, "rb");
    if (!fh) {
        fprintf(stderr, "cannot open %s\n", name);
        exit(2);
    }
    std::vector<uint8_t> f;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) f.insert(f.end(), buf, buf + got);
    fclose(fh);
    return f;
}

int main(int argc, char **argv)
{
    std::vector<std::string> good, packs;
    std::vector<int> sizes;
    int mode = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--subseq")) mode = 1;
        else if (!strcmp(argv[i], "--good")) mode = 2;
        else if (!strcmp(argv[i], "--pack")) mode = 3;
        else if (mode == 1) sizes.push_back(atoi(argv[i]));
        else if (mode == 2) good.push_back(argv[i]);
        else if (mode == 3) packs.push_back(argv[i]);
    }
    if (sizes.empty() || (good.empty() && packs.empty())) {
        fprintf(stderr, "usage: jpeg_entropy_emul --subseq S... [--good FILE...] [--pack PACKFILE...]\n");
        return 2;
    }
    for (int S : sizes)
        if (S < 16 || S > 1024 || (S & (S - 1))) {
            fprintf(stderr, "subsequence size %d is no power of two in 16..1024\n", S);
            return 2;
        }
    for (const std::string &name : good) {
        const std::vector<uint8_t> f = slurp(name.c_str());
        const size_t slash = name.find_last_of('/');
        for (int S : sizes) check(f, slash == std::string::npos ? name : name.substr(slash + 1), S, true);
    }
    for (const std::string &name : packs) {
        const std::vector<uint8_t> p = slurp(name.c_str());
        size_t at = 0;
        long rec = 0;
        while (at + 4 <= p.size()) {
            uint32_t len;
            memcpy(&len, p.data() + at, 4);
            at += 4;
            if (len > p.size() - at) {
                fprintf(stderr, "%s: record %ld runs past the end\n", name.c_str(), rec);
                return 2;
            }
            const std::vector<uint8_t> f(p.begin() + at, p.begin() + at + len);
            at += len;
            for (int S : sizes) check(f, name + "#" + std::to_string(rec), S, false);
            ++rec;
        }
    }
    printf("emulated %ld good files, %ld mutations (%ld accepted, %ld declined), %ld failures\n", n_good, n_mut, n_accepted, n_declined, failures);
    return failures ? 1 : 0;
}
