// Stand-alone driver of csrc/jpeg_host.cpp for a sanitizer build (tests/test_jpeg_host.py compiles both with
// g++ -fsanitize=address,undefined and runs the result as a child process):
//     jpeg_fuzz FILE... --seeds SEED...
// decodes every file, then a fixed, seeded set of mutations of each -- truncation at every 53rd byte, single-byte flips
// over the first 700 bytes, random 4-byte splices in the scan -- from heap buffers of exactly the right sizes, so that a
// read or write past either end is a sanitizer report.  Exit status 0: every original decoded with status 0 and nothing
// was reported.
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

static long counts[3];

// probe + entropy stage of one buffer; the file and the outputs live in exact-size heap blocks
static int decode(const std::vector<uint8_t> &file)
{
    uint8_t *data = (uint8_t *)malloc(file.size() ? file.size() : 1);
    if (!file.empty()) memcpy(data, file.data(), file.size());
    mmr_jpeg_info info;
    const int st = mmr_jpeg_probe(data, (int64_t)file.size(), &info);
    int32_t status = st;
    if (st == MMR_JPEG_OK) {
        int16_t *coef = (int16_t *)aligned_alloc(16, (size_t)(info.coef_bytes + 15) / 16 * 16);
        uint16_t *qt = (uint16_t *)malloc(192 * sizeof(uint16_t));
        const void *datas[1] = {data};
        const int64_t sizes[1] = {(int64_t)file.size()}, off[1] = {0};
        if (mmr_jpeg_entropy_decode(datas, sizes, 1, &info, coef, off, qt, &status, 1) != MMR_OK) {
            fprintf(stderr, "mmr_jpeg_entropy_decode rejected its arguments\n");
            exit(2);
        }
        free(coef);
        free(qt);
    }
    free(data);
    if (status < 0 || status > 2) {
        fprintf(stderr, "status %d is none of the three codes\n", status);
        exit(2);
    }
    ++counts[status];
    return status;
}

static size_t scan_start(const std::vector<uint8_t> &f)
{
    for (size_t i = 0; i + 1 < f.size(); ++i)
        if (f[i] == 0xFF && f[i + 1] == 0xDA) return i;
    return 0;
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
        fprintf(stderr, "usage: jpeg_fuzz FILE... --seeds SEED...\n");
        return 2;
    }
    std::vector<std::vector<uint8_t>> files;
    for (const std::string &name : names) {
        FILE *fh = fopen(name.c_str(), "rb");
        if (!fh) {
            fprintf(stderr, "cannot open %s\n", name.c_str());
            return 2;
        }
        std::vector<uint8_t> f;
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), fh)) > 0) f.insert(f.end(), buf, buf + got);
        fclose(fh);
        if (decode(f) != MMR_JPEG_OK) {
            fprintf(stderr, "%s does not decode\n", name.c_str());
            return 1;
        }
        files.push_back(f);
    }
    decode(std::vector<uint8_t>());
    for (const std::vector<uint8_t> &f : files) {
        for (size_t cut = 0; cut < f.size(); cut += 53) decode(std::vector<uint8_t>(f.begin(), f.begin() + cut));
        const size_t scan = scan_start(f);
        for (uint64_t seed : seeds) {
            rng_state = seed * 0x9E3779B97F4A7C15ull + f.size();
            for (size_t at = 0; at < f.size() && at < 700; ++at) {
                std::vector<uint8_t> m = f;
                m[at] ^= (uint8_t)(1 + rnd() % 255);
                decode(m);
            }
            for (int k = 0; k < 64 && scan + 8 < f.size(); ++k) {
                std::vector<uint8_t> m = f;
                const size_t at = scan + rnd() % (f.size() - scan - 4);
                for (int j = 0; j < 4; ++j) m[at + j] = (uint8_t)rnd();
                decode(m);
            }
        }
    }
    // the whole set in one threaded call, a file that is not a JPEG in the middle
    {
        std::vector<std::vector<uint8_t>> batch = files;
        batch.insert(batch.begin() + batch.size() / 2, std::vector<uint8_t>(100, 0x55));
        const int B = (int)batch.size();
        std::vector<mmr_jpeg_info> infos(B);
        std::vector<const void *> datas(B);
        std::vector<int64_t> sizes(B), off(B);
        int64_t total = 0;
        for (int i = 0; i < B; ++i) {
            datas[i] = batch[i].data();
            sizes[i] = (int64_t)batch[i].size();
            mmr_jpeg_probe(batch[i].data(), sizes[i], &infos[i]);
            off[i] = total;
            if (infos[i].status == MMR_JPEG_OK) total += infos[i].coef_bytes;
        }
        int16_t *coef = (int16_t *)aligned_alloc(16, (size_t)(total + 15) / 16 * 16);
        std::vector<uint16_t> qt((size_t)B * 192);
        std::vector<int32_t> status(B, -1);
        if (mmr_jpeg_entropy_decode(datas.data(), sizes.data(), B, infos.data(), coef, off.data(), qt.data(), status.data(), 4) != MMR_OK) return 2;
        free(coef);
        for (int i = 0; i < B; ++i)
            if ((status[i] == MMR_JPEG_OK) != (batch[i].size() != 100)) {
                fprintf(stderr, "batch row %d: status %d\n", i, status[i]);
                return 1;
            }
    }
    printf("decoded %ld ok, %ld unsupported, %ld corrupt\n", counts[0], counts[1], counts[2]);
    return 0;
}
