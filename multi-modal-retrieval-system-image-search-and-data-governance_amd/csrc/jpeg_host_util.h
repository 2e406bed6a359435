// What the two host stages of the JPEG path (jpeg_host.cpp, jpeg_encode_host.cpp) share beyond the layout in
// jpeg_geometry.h: how an argument error is reported and how a batch is spread over threads.  Plain C++17, no HIP call.
#pragma once
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/mmr.h"
#include "jpeg_geometry.h"

namespace mmr {
// api_common.cpp's; weak, so that the host stages link on their own (the error text is then dropped)
void set_error(const char *fmt, ...) __attribute__((weak));
}

namespace mmr_jpeg {

inline int fail(const char *msg)
{
    if (mmr::set_error) mmr::set_error("%s", msg);
    return MMR_EINVAL;
}

// row(i) for every i in [0, B), handed out one at a time to min(threads, B) threads, the caller among them
template <class Row>
void parallel_rows(int B, int threads, Row row)
{
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < B; i = next.fetch_add(1)) row(i);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads && t < B; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
}

}  // namespace mmr_jpeg
