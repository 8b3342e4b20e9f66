// fp_short_forms.hip -- device check of the short correctly rounded forms of csrc/device_math.h (rcp_rn, sqrt_rn, div_rn)
// against '/' and sqrtf of the same translation unit, compiled with the library's flags.  Bitwise comparison; two NaNs count
// as equal.  Prints one JSON object (tests/test_gpu_fp_short_forms.py reads it).
//
//   rcp_rn, sqrt_rn: every one of the 2^32 inputs; mismatches are counted per (sign, biased exponent) bucket.
//   div_rn: every divisor mantissa at a set of exponents against a table of numerators at the domain edges and with hard
//           mantissas, then random pairs inside the declared domain.  Pairs outside it are counted separately.
//
// Mismatches are counted per wave (ballot + popcount, or shuffles) and added with ordinary global atomics by one lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "device_math.h"

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

// The declared domains (device_math.h).
__device__ __forceinline__ bool rcp_domain(float b) {
    const float m = fabsf(b);
    return (m >= 0x1p-126f && m <= 0x1p126f) || m == 0.0f || m == __builtin_huge_valf() || b != b;
}
__device__ __forceinline__ bool sqrt_domain(float x) { return !(fabsf(x) > 0.0f && fabsf(x) < 0x1p-104f); }
__device__ __forceinline__ bool div_domain(float a, float b, float q) {
    const float ma = fabsf(a), mb = fabsf(b), mq = fabsf(q);
    return mb >= 0x1p-126f && mb <= 0x1p126f && (ma == 0.0f || (ma >= 0x1p-100f && mq >= 0x1p-126f && mq < 0x1p127f));
}

enum { F_RCP = 0, F_SQRT = 1 };
template <int F>
__device__ __forceinline__ bool unary(float x, float *got, float *want) {  // true: x is in the form's domain
    if (F == F_RCP) {
        *got = rcp_rn(x);
        *want = 1.0f / x;
        return rcp_domain(x);
    } else {
        *got = sqrt_rn(x);
        *want = sqrtf(x);
        return sqrt_domain(x);
    }
}

// one launch: 2^28 consecutive inputs from base, 16 per thread; a wave always covers 64 inputs of one bucket (bits >> 23).
// hist[0..511]: mismatches per bucket, hist[512]: mismatches inside the domain
template <int F>
__global__ void __launch_bounds__(256) k_unary(uint32_t base, unsigned long long *hist, uint32_t *example) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint32_t bits = base + k * stride + tid;
        float got, want;
        const bool in = unary<F>(__uint_as_float(bits), &got, &want);
        const bool bad = !same(got, want);
        const unsigned long long m = __ballot(bad), m_in = __ballot(bad && in);
        if (m != 0ull && lane == 0u) {
            atomicAdd(&hist[bits >> 23], (unsigned long long)__popcll(m));
            atomicMax(&example[bits >> 23], bits + 63u - (uint32_t)__clzll(m));
            if (m_in) atomicAdd(&hist[512], (unsigned long long)__popcll(m_in));
        }
    }
}

// counters of the division check: [0] pairs in the domain, [1] their mismatches, [2] pairs outside it, [3] their mismatches;
// kept per lane and added up per wave at the end of a thread's pairs
struct DivCount {
    uint32_t c[4];
};
__device__ __forceinline__ void count_div(float a, float b, DivCount &n, uint32_t *example) {
    const float want = a / b, got = div_rn(a, b);
    const bool in = div_domain(a, b, want), bad = !same(got, want);
    n.c[0] += in;
    n.c[1] += in && bad;
    n.c[2] += !in;
    n.c[3] += !in && bad;
    if (in && bad) {  // one in-domain counterexample (a, b), whichever lane writes last
        example[0] = __float_as_uint(a);
        example[1] = __float_as_uint(b);
    }
}
__device__ __forceinline__ void flush_div(const DivCount &n, unsigned long long *c) {
    for (int i = 0; i < 4; ++i) {
        uint32_t v = n.c[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&c[i], (unsigned long long)v);
    }
}

// every divisor mantissa (2^23 threads) with biased exponent eb, against numerators num[0..n)
__global__ void __launch_bounds__(256) k_div_grid(uint32_t eb, const float *num, uint32_t n, unsigned long long *c, uint32_t *example) {
    const uint32_t mant = blockIdx.x * blockDim.x + threadIdx.x;
    const float b = __uint_as_float((eb << 23) | mant);
    DivCount k = {{0, 0, 0, 0}};
    for (uint32_t i = 0; i < n; ++i) {
        count_div(num[i], b, k, example);
        count_div(num[i], -b, k, example);
    }
    flush_div(k, c);
}

__device__ __forceinline__ uint32_t hash(uint32_t x) {  // lowbias32
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// random pairs: the divisor's exponent in [-126, 126], the numerator's in [-100, 127] with a quotient exponent in [-126, 127],
// random signs and mantissas; the few whose quotient still leaves the normal range are counted as outside the domain
__global__ void __launch_bounds__(256) k_div_random(uint32_t launch, unsigned long long *c, uint32_t *example) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = hash(tid ^ hash(launch * 0x9e3779b9u + 1u));
    DivCount n = {{0, 0, 0, 0}};
    for (uint32_t k = 0; k < 64u; ++k) {
        const uint32_t r0 = hash(s += 0x632be5abu), r1 = hash(s += 0x632be5abu), r2 = hash(s += 0x632be5abu);
        const int eb = (int)((r2 & 0xffffu) % 253u) - 126;  // [-126, 126]
        const int lo = max(-100, eb - 126), hi = min(127, eb + 127);  // the quotient's exponent stays in [-126, 127]
        const int ea = lo + (int)((r2 >> 16) % (uint32_t)(hi - lo + 1));
        const float b = __uint_as_float((r0 & 0x807fffffu) | ((uint32_t)(eb + 127) << 23));
        const float a = __uint_as_float((r1 & 0x807fffffu) | ((uint32_t)(ea + 127) << 23));
        count_div(a, b, n, example);
    }
    flush_div(n, c);
}

static float f_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    const int nb = 65536, nt = 256;  // 2^24 threads
    unsigned long long *d_hist;
    uint32_t *d_ex;
    CHECK(hipMalloc(&d_hist, 513 * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_ex, 512 * sizeof(uint32_t)));
    printf("{");
    const char *names[2] = {"rcp_rn", "sqrt_rn"};
    for (int f = 0; f < 2; ++f) {
        CHECK(hipMemset(d_hist, 0, 513 * sizeof(unsigned long long)));
        CHECK(hipMemset(d_ex, 0, 512 * sizeof(uint32_t)));
        for (uint32_t l = 0; l < 16u; ++l) {
            if (f == F_RCP)
                hipLaunchKernelGGL(k_unary<F_RCP>, dim3(nb), dim3(nt), 0, 0, l << 28, d_hist, d_ex);
            else
                hipLaunchKernelGGL(k_unary<F_SQRT>, dim3(nb), dim3(nt), 0, 0, l << 28, d_hist, d_ex);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
        }
        unsigned long long hist[513];
        uint32_t ex[512];
        CHECK(hipMemcpy(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(ex, d_ex, sizeof(ex), hipMemcpyDeviceToHost));
        unsigned long long total = 0;
        for (int i = 0; i < 512; ++i) total += hist[i];
        // buckets: "sign,biased exponent": [mismatches, one mismatching input as hex]
        printf("\"%s\": {\"inputs\": 4294967296, \"mismatches\": %llu, \"domain_mismatches\": %llu, \"buckets\": {", names[f], total,
               hist[512]);
        bool first = true;
        for (int i = 0; i < 512; ++i) {
            if (!hist[i]) continue;
            printf("%s\"%d,%d\": [%llu, \"0x%08x\"]", first ? "" : ", ", i >> 8, i & 255, hist[i], ex[i]);
            first = false;
        }
        printf("}}, ");
        fflush(stdout);
    }

    // numerators of the grid check: domain edges, hard mantissas, zeros, and 0 / inf / NaN / tiny ones outside the domain
    std::vector<float> num;
    const uint32_t mants[] = {0x000000u, 0x000001u, 0x000002u, 0x7fffffu, 0x7ffffeu, 0x400000u, 0x3fffffu, 0x400001u, 0x555555u,
                              0x2aaaaau, 0x5db3d7u, 0x0ccccdu, 0x490fdbu, 0x35040u,  0x6a09e6u, 0x7ff000u};
    const int exps[] = {-100, -99, -64, -24, -2, -1, 0, 1, 2, 23, 64, 100, 126, 127};
    for (int e : exps)
        for (uint32_t m : mants) {
            num.push_back(f_of(((uint32_t)(e + 127) << 23) | m));
            num.push_back(-f_of(((uint32_t)(e + 127) << 23) | m));
        }
    uint32_t s = 12345u;
    while (num.size() < 2048) {  // random mantissas at random exponents in [-100, 127]
        s = s * 1664525u + 1013904223u;
        const uint32_t m = s >> 9;
        s = s * 1664525u + 1013904223u;
        num.push_back(f_of((s & 0x80000000u) | ((27u + (s >> 8) % 228u) << 23) | m));
    }
    num.push_back(0.0f);
    num.push_back(-0.0f);
    float *d_num;
    unsigned long long *d_c;
    CHECK(hipMalloc(&d_num, num.size() * sizeof(float)));
    CHECK(hipMalloc(&d_c, 4 * sizeof(unsigned long long)));
    CHECK(hipMemcpy(d_num, num.data(), num.size() * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_c, 0, 4 * sizeof(unsigned long long)));
    CHECK(hipMemset(d_ex, 0, 2 * sizeof(uint32_t)));
    const int div_exps[] = {-126, -125, -100, -64, -1, 0, 1, 64, 100, 125, 126};  // unbiased exponents of the divisor
    const uint32_t per_launch = 256;  // numerators per launch: 2^23 x 2 x 256 = 4.3e9 pairs
    for (int e : div_exps)
        for (uint32_t i = 0; i < num.size(); i += per_launch) {
            const uint32_t n = (uint32_t)num.size() - i < per_launch ? (uint32_t)num.size() - i : per_launch;
            hipLaunchKernelGGL(k_div_grid, dim3((1u << 23) / 256u), dim3(256), 0, 0, (uint32_t)(e + 127), d_num + i, n, d_c, d_ex);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
        }
    unsigned long long c[4];
    uint32_t ex[2];
    CHECK(hipMemcpy(c, d_c, sizeof(c), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ex, d_ex, sizeof(ex), hipMemcpyDeviceToHost));
    printf("\"div_rn_grid\": {\"numerators\": %zu, \"divisor_exponents\": %zu, \"in_domain\": %llu, \"mismatches\": %llu, "
           "\"outside\": %llu, \"outside_mismatches\": %llu, \"example\": [\"0x%08x\", \"0x%08x\"]}, ",
           num.size(), sizeof(div_exps) / sizeof(int), c[0], c[1], c[2], c[3], ex[0], ex[1]);
    fflush(stdout);

    CHECK(hipMemset(d_c, 0, 4 * sizeof(unsigned long long)));
    CHECK(hipMemset(d_ex, 0, 2 * sizeof(uint32_t)));
    const uint32_t launches = 12;  // 2^24 threads x 64 pairs x 12 = 1.29e10 pairs
    for (uint32_t l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(k_div_random, dim3(nb), dim3(nt), 0, 0, l, d_c, d_ex);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(c, d_c, sizeof(c), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ex, d_ex, sizeof(ex), hipMemcpyDeviceToHost));
    printf("\"div_rn_random\": {\"in_domain\": %llu, \"mismatches\": %llu, \"outside\": %llu, \"outside_mismatches\": %llu, "
           "\"example\": [\"0x%08x\", \"0x%08x\"]}}\n",
           c[0], c[1], c[2], c[3], ex[0], ex[1]);
    CHECK(hipFree(d_num));
    CHECK(hipFree(d_c));
    CHECK(hipFree(d_hist));
    CHECK(hipFree(d_ex));
    return 0;
}
