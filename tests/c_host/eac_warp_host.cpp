// eac_warp_host.cpp - the HOST build of csrc/pb_eac.hpp, the two functions that make a cube map equi-angular: the very text
// the device compiles.  Prints, for each face size N given on the command line, the result bits of pb_eac_warp on every mesh value
// linspace(-N/2 + 0.5, N/2 - 0.5, N) and of pb_eac_unwarp on a seeded sweep of [-N/2, N/2] - one line per value, "w N <argument bits>
// <result bits>" / "u N ...", hexadecimal - for tests/test_eac_host.py to compare with NumPy's.  Compile with -ffp-contract=off -mfma,
// plain (NumPy's SIMD kernels) and with -DPB_MATH_LIBM (glibc's functions, what NumPy calls without AVX512_SKX).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../photonbend_amd/csrc/pb_eac.hpp"

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

// the sweep's arguments: a 64-bit LCG (Knuth's MMIX constants), the top 53 bits as a fraction of [-half, half]
static uint64_t lcg(uint64_t& s) { return s = s * 6364136223846793005ull + 1442695040888963407ull; }

int main(int argc, char** argv) {
    const int sweep = 4096;
    for (int a = 1; a < argc; ++a) {
        const int n = std::atoi(argv[a]);
        if (n < 1) return 2;
        const double half = (double)n / 2;
        const double start = -half + 0.5, stop = half - 0.5;
        const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
        for (int k = 0; k < n; ++k) {
            const double c = (k == n - 1 && n > 1) ? stop : (double)k * step + start;  // np.linspace
            std::printf("w %d %016llx %016llx\n", n, (unsigned long long)bits_of(c), (unsigned long long)bits_of(pb_eac_warp(c, half)));
        }
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        for (int k = 0; k < sweep; ++k) {
            const double u = (double)(lcg(s) >> 11) * 0x1p-53;  // [0, 1)
            const double c = k == 0 ? -half : (k == 1 ? half : (k == 2 ? 0.0 : (u * 2.0 - 1.0) * half));
            std::printf("u %d %016llx %016llx\n", n, (unsigned long long)bits_of(c), (unsigned long long)bits_of(pb_eac_unwarp(c, half)));
        }
    }
    return 0;
}
