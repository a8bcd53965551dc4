// dl_philox.h -- the counter-based generator every device-resident sampler draws from (dl_ens_fold.h, dl_mh.h, dl_nuts.h): Philox4x32-10 and the 53-bit uniform of
// two words, the Box-Muller Gaussians of one block.  Free of HIP headers, so that the host build of a sampler's arithmetic (tests/csrc) compiles the same functions.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DL_PHILOX_HD __host__ __device__ inline
#else
#define DL_PHILOX_HD inline
#endif

struct DlPhilox {
    uint32_t x[4];
};

// Philox4x32-10 (Random123): counter c[4], key k[2]
DL_PHILOX_HD DlPhilox dl_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return DlPhilox{{c0, c1, c2, c3}};
}

// 53-bit uniform on [0, 1) from two 32-bit words (the construction of numpy's random_sample)
DL_PHILOX_HD double dl_uniform53(uint32_t hi, uint32_t lo) { return ((double)(hi >> 5) * 67108864. + (double)(lo >> 6)) * (1. / 9007199254740992.); }

// standard Gaussian i of the Box-Muller pair of one block: radius from words 0, 1, angle from words 2, 3; even i the cosine, odd i the sine
DL_PHILOX_HD double dl_box_muller(const DlPhilox& r, int i) {
    const double rad = sqrt(-2. * log1p(-dl_uniform53(r.x[0], r.x[1]))), ang = 6.283185307179586 * dl_uniform53(r.x[2], r.x[3]);
    return (i & 1) ? rad * sin(ang) : rad * cos(ang);
}
