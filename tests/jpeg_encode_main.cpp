// Stand-alone driver of csrc/jpeg_encode_host.cpp for a sanitizer build (tests/test_jpeg_encode_host.py compiles it, the
// encoder and csrc/jpeg_host.cpp with g++ -fsanitize=address,undefined and runs the result as a child process):
//     jpeg_encode_main FILE... --seeds SEED...
// Every file (a golden written by Pillow with the standard tables) is decoded to coefficients and coded again: the bytes
// must be the file's.  Then the same coefficients, and seeded random blocks over several geometries and magnitudes (some
// outside what the baseline tables can code), are coded into heap buffers of EXACTLY the capacity passed, for capacities
// from 0 to mmr_jpeg_encode_bound, so that a write past the capacity is a sanitizer report.  Exit status 0: every golden
// came back byte for byte, every status was one of the documented ones, and nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/mmr.h"

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static long counts[5];

// one image into an exact-size heap buffer; returns the status, the file in `got` when it is 0
static int encode(const mmr_jpeg_info &info, const int16_t *coef, const uint16_t *qt, int restart, int64_t cap, std::vector<uint8_t> *got)
{
    uint8_t *out = (uint8_t *)malloc(cap ? (size_t)cap : 1);
    const int64_t off[1] = {0}, caps[1] = {cap};
    int64_t size = -1;
    int32_t status = -1;
    if (mmr_jpeg_entropy_encode(coef, off, &info, qt, 1, restart, out, off, caps, &size, &status, 1) != MMR_OK) {
        fprintf(stderr, "mmr_jpeg_entropy_encode rejected its arguments\n");
        exit(2);
    }
    const bool sane = status == MMR_JPEG_OK ? (size > 0 && size <= cap) : ((status == MMR_JPEG_NO_ROOM || status == MMR_JPEG_UNSUPPORTED) && size == 0);
    if (!sane) {
        fprintf(stderr, "status %d with %lld bytes in a capacity of %lld\n", status, (long long)size, (long long)cap);
        exit(1);
    }
    if (got && status == MMR_JPEG_OK) got->assign(out, out + size);
    free(out);
    ++counts[status];
    return status;
}

static mmr_jpeg_info geometry(int H, int W, int ncomp, int hmax, int vmax)
{
    mmr_jpeg_info f;
    memset(&f, 0, sizeof(f));
    f.W = W; f.H = H; f.ncomp = ncomp; f.hmax = hmax; f.vmax = vmax;
    f.mcus_x = (W + 8 * hmax - 1) / (8 * hmax);
    f.mcus_y = (H + 8 * vmax - 1) / (8 * vmax);
    f.blocks0 = f.mcus_x * f.mcus_y * hmax * vmax;
    f.blocks1 = f.blocks2 = ncomp == 3 ? f.mcus_x * f.mcus_y : 0;
    f.coef_bytes = ((int64_t)f.blocks0 + f.blocks1 + f.blocks2) * 128;
    return f;
}

int main(int argc, char **argv)
{
    std::vector<std::string> names;
    std::vector<uint64_t> seeds;
    bool in_seeds = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--seeds")) in_seeds = true;
        else if (in_seeds) seeds.push_back(strtoull(argv[i], nullptr, 10));
        else names.push_back(argv[i]);
    }
    if (names.empty() || seeds.empty()) {
        fprintf(stderr, "usage: jpeg_encode_main FILE... --seeds SEED...\n");
        return 2;
    }
    for (const std::string &name : names) {
        FILE *fh = fopen(name.c_str(), "rb");
        if (!fh) {
            fprintf(stderr, "cannot open %s\n", name.c_str());
            return 2;
        }
        std::vector<uint8_t> f;
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), fh)) > 0) f.insert(f.end(), buf, buf + n);
        fclose(fh);
        mmr_jpeg_info info;
        if (mmr_jpeg_probe(f.data(), (int64_t)f.size(), &info) != MMR_JPEG_OK) {
            fprintf(stderr, "%s does not probe\n", name.c_str());
            return 1;
        }
        int16_t *coef = (int16_t *)aligned_alloc(16, (size_t)(info.coef_bytes + 15) / 16 * 16);
        uint16_t qt[192];
        const void *datas[1] = {f.data()};
        const int64_t sizes[1] = {(int64_t)f.size()}, off[1] = {0};
        int32_t status = -1;
        if (mmr_jpeg_entropy_decode(datas, sizes, 1, &info, coef, off, qt, &status, 1) != MMR_OK || status != MMR_JPEG_OK) {
            fprintf(stderr, "%s does not decode\n", name.c_str());
            return 1;
        }
        int restart = 0;
        for (size_t i = 0; i + 5 < f.size(); ++i)
            if (f[i] == 0xFF && f[i + 1] == 0xDD) { restart = (f[i + 4] << 8) | f[i + 5]; break; }
            else if (f[i] == 0xFF && f[i + 1] == 0xDA) break;
        const int64_t bound = mmr_jpeg_encode_bound(&info), len = (int64_t)f.size();
        std::vector<uint8_t> got;
        if (bound < len || encode(info, coef, qt, restart, bound, &got) != MMR_JPEG_OK || got != f) {
            fprintf(stderr, "%s: coded again, the bytes are not the file's (bound %lld, file %lld, got %zu)\n", name.c_str(), (long long)bound, (long long)len, got.size());
            return 1;
        }
        got.clear();
        if (encode(info, coef, qt, restart, len, &got) != MMR_JPEG_OK || got != f) {
            fprintf(stderr, "%s: does not fit a capacity of exactly its length\n", name.c_str());
            return 1;
        }
        for (int64_t cap = 0; cap < len; cap += (cap < 700 ? 1 : 37))
            if (encode(info, coef, qt, restart, cap, nullptr) != MMR_JPEG_NO_ROOM) {
                fprintf(stderr, "%s: capacity %lld of %lld did not answer MMR_JPEG_NO_ROOM\n", name.c_str(), (long long)cap, (long long)len);
                return 1;
            }
        if (encode(info, coef, qt, restart, len - 1, nullptr) != MMR_JPEG_NO_ROOM) return 1;
        free(coef);
    }
    // seeded random blocks: magnitudes from what a quantiser gives to the whole int16 range
    static const int geo[][5] = {{1, 1, 1, 1, 1}, {1, 1, 3, 2, 2}, {9, 3, 3, 2, 1}, {17, 33, 3, 1, 1}, {24, 40, 3, 2, 2}, {37, 51, 1, 1, 1}};
    static const int magnitude[] = {2, 16, 255, 1023, 1024, 2047, 32767};
    uint16_t qt[192];
    for (uint64_t seed : seeds) {
        rng_state = seed * 0x9E3779B97F4A7C15ull + 12345;
        for (const auto &g : geo)
            for (int mag : magnitude)
                for (int density = 0; density < 3; ++density) {
                    const mmr_jpeg_info info = geometry(g[0], g[1], g[2], g[3], g[4]);
                    const size_t ncoef = (size_t)info.coef_bytes / 2;
                    int16_t *coef = (int16_t *)malloc(ncoef * sizeof(int16_t));
                    for (size_t i = 0; i < ncoef; ++i) {
                        const bool on = density == 2 || rnd() % (density ? 3 : 17) == 0;
                        coef[i] = on ? (int16_t)((int)(rnd() % (2 * mag + 1)) - mag) : 0;
                    }
                    for (int i = 0; i < 192; ++i) qt[i] = (uint16_t)(1 + rnd() % 255);
                    const int restart = (int)(rnd() % 4);
                    const int64_t bound = mmr_jpeg_encode_bound(&info);
                    std::vector<uint8_t> whole;
                    const int st = encode(info, coef, qt, restart, bound, &whole);
                    if (st == MMR_JPEG_NO_ROOM) {
                        fprintf(stderr, "the bound of %lld bytes was too small\n", (long long)bound);
                        return 1;
                    }
                    if ((mag <= 1023 && st != MMR_JPEG_OK) || (mag == 32767 && density == 2 && st != MMR_JPEG_UNSUPPORTED)) {
                        fprintf(stderr, "coefficients up to %d, density %d: status %d\n", mag, density, st);
                        return 1;
                    }
                    for (int k = 0; k < 24; ++k) {
                        const int64_t cap = k == 0 ? 0 : (int64_t)(rnd() % (uint32_t)(bound + 1));
                        std::vector<uint8_t> part;
                        const int s2 = encode(info, coef, qt, restart, cap, &part);
                        if (st == MMR_JPEG_OK && (s2 == MMR_JPEG_OK) != (cap >= (int64_t)whole.size())) {
                            fprintf(stderr, "capacity %lld against a file of %zu bytes: status %d\n", (long long)cap, whole.size(), s2);
                            return 1;
                        }
                        if (s2 == MMR_JPEG_OK && part != whole) return 1;
                    }
                    free(coef);
                }
    }
    // a threaded batch whose middle row has no room: its neighbours are whole
    {
        const mmr_jpeg_info info = geometry(24, 40, 3, 2, 2);
        const int B = 7;
        const size_t ncoef = (size_t)info.coef_bytes / 2;
        std::vector<int16_t> coef(ncoef * B);
        for (auto &c : coef) c = rnd() % 5 == 0 ? (int16_t)((int)(rnd() % 201) - 100) : 0;
        std::vector<uint16_t> qts((size_t)B * 192, 3);
        std::vector<mmr_jpeg_info> infos(B, info);
        std::vector<int64_t> coff(B), ooff(B), caps(B), sizes(B, -1);
        std::vector<int32_t> status(B, -1);
        const int64_t bound = mmr_jpeg_encode_bound(&info);
        int64_t at = 0;
        for (int i = 0; i < B; ++i) {
            coff[i] = (int64_t)(ncoef * 2 * i);
            caps[i] = i == 3 ? 100 : bound;
            ooff[i] = at;
            at += caps[i];
        }
        uint8_t *out = (uint8_t *)malloc((size_t)at);
        if (mmr_jpeg_entropy_encode(coef.data(), coff.data(), infos.data(), qts.data(), B, 0, out, ooff.data(), caps.data(), sizes.data(), status.data(), 4) != MMR_OK) return 2;
        for (int i = 0; i < B; ++i) {
            std::vector<uint8_t> alone;
            encode(info, coef.data() + ncoef * i, qts.data(), 0, bound, &alone);
            const bool ok = i == 3 ? (status[i] == MMR_JPEG_NO_ROOM && sizes[i] == 0)
                                   : (status[i] == MMR_JPEG_OK && sizes[i] == (int64_t)alone.size() && !memcmp(out + ooff[i], alone.data(), alone.size()));
            if (!ok) {
                fprintf(stderr, "batch row %d: status %d, %lld bytes\n", i, status[i], (long long)sizes[i]);
                return 1;
            }
        }
        free(out);
    }
    printf("encoded %ld ok, %ld unsupported, %ld without room\n", counts[0], counts[1], counts[4]);
    return 0;
}
