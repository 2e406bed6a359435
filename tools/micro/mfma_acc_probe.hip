// Micro-probe (development aid, not part of the library): the fp32 accumulation error of the MFMA shapes the gallery
// scans run on -- v_mfma_f32_32x32x16 and v_mfma_f32_16x16x32, each in its f16 and its bf16 form -- over chains of
// E = 1024 elements, the longest rows the search takes.  The scans' certificate (search.hip: rank_kernel, range_common.h:
// scan_margin) allows |acc - dot64| <= 8e-5 * |q| * |g|; that figure was sized for the bf16 instructions.  This prints
//     max |acc - dot64| / (|q| |g|)
// per instruction and operand pattern, so the fp16 scans' margin rests on a measurement of the f16 adder and not on the
// assumption that it is the bf16 one.  Every operand is exactly representable in BOTH formats (8 significant bits,
// exponents inside fp16's normal range), so the two forms multiply the same numbers and the products are exact:
//     same sign     every product positive: the sum grows, each add rounds at the running sum's ulp
//     alternating   signs alternate along k: cancellation, error relative to the norms
//     huge + small  one product of 2^12 first, 1023 small ones behind it: every add rounds at the huge term's ulp (the
//                   worst case for a chained accumulator: up to E/2 ulp if it rounds to nearest, E ulp if it truncates)
// One accumulation chain per tile (the scans use one or two); 32 (16) rows x 32 (16) queries per case, 64 cases.
// Last line: fp16 SUBNORMAL operands (2^-24 .. 2^-15) against ones -- whether the f16 MFMA keeps them under the
// kernel's float_denorm_mode_16_64 = 3 or flushes them to zero.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_acc_probe.hip -o mfma_acc_probe && ./mfma_acc_probe > profiles/mfma_acc_probe.txt
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) short bits16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int E = 1024;

// one wave per case: rows[case][32][E] x cols[case][32][E] -> out[case][row][col], one chain of E/16 MFMAs.
// Lane (c = lane & 31, h = lane >> 5) holds elements [16s + 8h, +8) of row c (A) and of column c (B);
// acc[i] = dot(col c, row (i&3) + 8*(i>>2) + 4h).
template <bool F16>
__global__ __launch_bounds__(64) void chain_32x32x16(const uint16_t *__restrict__ rows, const uint16_t *__restrict__ cols,
                                                     float *__restrict__ out)
{
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const uint16_t *a = rows + ((size_t)blockIdx.x * 32 + c) * E + 8 * h;
    const uint16_t *b = cols + ((size_t)blockIdx.x * 32 + c) * E + 8 * h;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int s = 0; s < E / 16; ++s) {
        const bits16x8 av = *reinterpret_cast<const bits16x8 *>(a + 16 * s), bv = *reinterpret_cast<const bits16x8 *>(b + 16 * s);
        if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[((size_t)blockIdx.x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + c] = acc[i];
}

// the 16x16x32 form: the case's first 16 rows and columns.  Lane (c = lane & 15, g = lane >> 4) holds elements
// [32s + 8g, +8); acc[i] = dot(col c, row 4g + i).  Output in the same [32][32] block, entries [0,16) x [0,16).
template <bool F16>
__global__ __launch_bounds__(64) void chain_16x16x32(const uint16_t *__restrict__ rows, const uint16_t *__restrict__ cols,
                                                     float *__restrict__ out)
{
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const uint16_t *a = rows + ((size_t)blockIdx.x * 32 + c) * E + 8 * g;
    const uint16_t *b = cols + ((size_t)blockIdx.x * 32 + c) * E + 8 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < E / 32; ++s) {
        const bits16x8 av = *reinterpret_cast<const bits16x8 *>(a + 32 * s), bv = *reinterpret_cast<const bits16x8 *>(b + 32 * s);
        if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out[((size_t)blockIdx.x * 32 + 4 * g + i) * 32 + c] = acc[i];
}

// value = m * 2^e with |m| < 256: bits in both formats (host side, exact by construction)
static uint16_t to_bf16(float v) { uint32_t u; memcpy(&u, &v, 4); return (uint16_t)(u >> 16); }
static uint16_t to_f16(float v) { const _Float16 h = (_Float16)v; uint16_t u; memcpy(&u, &h, 2); return u; }

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main()
{
    constexpr int CASES = 64, R = 32;
    const size_t n = (size_t)CASES * R * E;
    std::vector<float> rowv(n), colv(n);
    std::vector<uint16_t> hb(n);
    uint16_t *drows, *dcols;
    float *dout;
    CHECK(hipMalloc(&drows, n * 2));
    CHECK(hipMalloc(&dcols, n * 2));
    CHECK(hipMalloc(&dout, (size_t)CASES * R * R * 4));
    std::vector<float> hout((size_t)CASES * R * R);

    // operand = m * 2^e, m in [128, 256) (8 significant bits), e so that |x| is in [2^-6, 2^-3): squares sum to O(1) rows
    auto small = [&]() { return (float)(128 + (int)(rng() % 128)) * exp2f(-13.f + (float)(rng() % 3)); };
    const char *names[] = {"same sign", "alternating", "huge + small", "fp16 subnormal operands x ones"};
    printf("%-32s %-24s %14s %14s\n", "pattern (E = 1024)", "instruction", "max rel err", "mean rel err");
    double worst[2] = {0.0, 0.0};        // [bf16, f16] over the three accumulation patterns
    for (int pat = 0; pat < 4; ++pat) {
        for (size_t i = 0; i < n; ++i) {
            const int k = (int)(i % E);
            float r = small(), c = small();
            if (pat == 1) { if (k & 1) r = -r; }                                   // products alternate in sign
            if (pat == 2) { if (k == 0) { r = 64.f; c = 64.f; } }                  // 2^12 first, then ~2^-9 each
            if (pat == 3) { r = (float)(1 + (int)(rng() % 512)) * 0x1p-24f; c = 1.f; }   // fp16 subnormals and 2^-15
            rowv[i] = r; colv[i] = c;
        }
        for (int f16 = 0; f16 < 2; ++f16) {
            if (pat == 3 && !f16) continue;
            for (size_t i = 0; i < n; ++i) hb[i] = f16 ? to_f16(rowv[i]) : to_bf16(rowv[i]);
            CHECK(hipMemcpy(drows, hb.data(), n * 2, hipMemcpyHostToDevice));
            for (size_t i = 0; i < n; ++i) hb[i] = f16 ? to_f16(colv[i]) : to_bf16(colv[i]);
            CHECK(hipMemcpy(dcols, hb.data(), n * 2, hipMemcpyHostToDevice));
            for (int shape = 0; shape < 2; ++shape) {
                const int dim = shape ? 16 : 32;
                CHECK(hipMemset(dout, 0, hout.size() * 4));
                if (shape == 0 && f16) hipLaunchKernelGGL(chain_32x32x16<true>, dim3(CASES), dim3(64), 0, 0, drows, dcols, dout);
                if (shape == 0 && !f16) hipLaunchKernelGGL(chain_32x32x16<false>, dim3(CASES), dim3(64), 0, 0, drows, dcols, dout);
                if (shape == 1 && f16) hipLaunchKernelGGL(chain_16x16x32<true>, dim3(CASES), dim3(64), 0, 0, drows, dcols, dout);
                if (shape == 1 && !f16) hipLaunchKernelGGL(chain_16x16x32<false>, dim3(CASES), dim3(64), 0, 0, drows, dcols, dout);
                CHECK(hipGetLastError());
                CHECK(hipMemcpy(hout.data(), dout, hout.size() * 4, hipMemcpyDeviceToHost));
                double mx = 0.0, sum = 0.0;
                size_t cnt = 0;
                for (int cs = 0; cs < CASES; ++cs)
                    for (int r = 0; r < dim; ++r)
                        for (int c = 0; c < dim; ++c) {
                            const float *pr = &rowv[((size_t)cs * R + r) * E], *pc = &colv[((size_t)cs * R + c) * E];
                            double d = 0.0, nr = 0.0, nc = 0.0;
                            for (int k = 0; k < E; ++k) { d += (double)pr[k] * pc[k]; nr += (double)pr[k] * pr[k]; nc += (double)pc[k] * pc[k]; }
                            const double rel = fabs((double)hout[((size_t)cs * R + r) * R + c] - d) / sqrt(nr * nc);
                            mx = rel > mx ? rel : mx; sum += rel; ++cnt;
                        }
                char ins[64];
                snprintf(ins, sizeof ins, "v_mfma_f32_%s_%s", shape ? "16x16x32" : "32x32x16", f16 ? "f16" : "bf16");
                printf("%-32s %-24s %14.3e %14.3e\n", names[pat], ins, mx, sum / (double)cnt);
                if (pat < 3 && mx > worst[f16]) worst[f16] = mx;
            }
        }
    }
    printf("worst case over the accumulation patterns: bf16 %.3e, f16 %.3e, ratio f16 / bf16 %.3f (margin in use: 8e-5)\n",
           worst[0], worst[1], worst[1] / worst[0]);
    printf("(fp16 subnormal row: a relative error near 1 means the operands were flushed to zero; ~1e-7 means they were kept)\n");
    return 0;
}
