// dl_ens_draw.h -- the stretch move's random draws as PURE functions of (key, iteration, half-step, slot): the random split of an ensemble, the draws of an accept
// and of a proposal, and the LDS-DMA staging of a step kernel's state.  ONE definition for the step kernel of a single ensemble (dl_ensemble.hip), the kernels of
// its folded update (dl_ens_fold.h: dl_kernels.hip, dl_chi2_gemm.h) and the step kernel of many ensembles bound to the vectors of a data batch
// (dl_ensemble_data.hip): an ensemble of the latter draws what a dl_ensemble with the same key draws.  Arithmetic is the NumPy driver's (samplers.py
// EnsembleStretchMove with CounterRNG), operation by operation (fp contraction off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dl_philox.h"   // dl_philox4x32, dl_uniform53

enum { DL_ENS_STREAM_PERM = 0, DL_ENS_STREAM_MOVE = 1, DL_ENS_STREAM_ACCEPT = 3 };   // + half-step for the last two

// LDS a step kernel may ask for (one workgroup; 160 KB per CU): dl_ens_launch keeps a single ensemble's state in LDS up to here, dl_ensemble_data_create refuses beyond
#define DL_ENS_LDS_BUDGET (144 * 1024)

// Random split of the ensemble into two halves: position r holds walker F(r), F a keyed bijection of [0, nw) -- four rounds of (odd multiplier, offset) mod 2^m
// and a right xor-shift, m = bit length of nw - 1, keyed by eight Philox words of the iteration, cycle-walked back into [0, nw).  Every element is a pure function
// of (seed, iteration, r): nothing is ranked, stored or exchanged.  The keys of a launch are made on the host and travel in the kernel arguments (dl_ensemble.hip),
// or by every workgroup from its own ensemble's key (dl_ensemble_data.hip): the function is the same on both sides.
// samplers.py CounterRNG.permutation is the NumPy statement of the same map.  F is inverted round by round (the xor-shift by >= m / 2 bits is an involution, the
// multipliers are odd: their inverses mod 2^32 are made with the keys), cycle-walking the inverse: position of walker w = F^-1(w).
struct DlEnsSplit {
    uint32_t mul[4], add[4], inv[4], mask, shift, nw;
};

DL_PHILOX_HD DlEnsSplit dl_ens_split(long long iteration, int nw, uint32_t k0, uint32_t k1) {
    const DlPhilox ka = dl_philox4x32((uint32_t)iteration, (uint32_t)((unsigned long long)iteration >> 32), 0u, DL_ENS_STREAM_PERM, k0, k1);
    const DlPhilox kb = dl_philox4x32((uint32_t)iteration, (uint32_t)((unsigned long long)iteration >> 32), 1u, DL_ENS_STREAM_PERM, k0, k1);
    DlEnsSplit f;
    int m = 1;
    while (m < 31 && (1u << m) < (uint32_t)nw) ++m;
    for (int round = 0; round < 4; ++round) {
        f.mul[round] = ka.x[round] | 1u; f.add[round] = kb.x[round];
        uint32_t inv = f.mul[round];                      // Newton: x <- x (2 - a x) doubles the number of correct low bits (3 to start with: a a = 1 mod 8)
        for (int it = 0; it < 5; ++it) inv *= 2u - f.mul[round] * inv;
        f.inv[round] = inv;
    }
    f.mask = (1u << m) - 1u; f.shift = (uint32_t)(m + 1) / 2; f.nw = (uint32_t)nw;
    return f;
}

__device__ __forceinline__ int dl_ens_split_at(const DlEnsSplit& f, int r) {
    uint32_t x = (uint32_t)r;
    do {
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            x = (x * f.mul[round] + f.add[round]) & f.mask;
            x ^= x >> f.shift;
        }
    } while (x >= f.nw);
    return (int)x;
}

// position r with dl_ens_split_at(f, r) == w
__device__ __forceinline__ int dl_ens_split_inv(const DlEnsSplit& f, int w) {
    uint32_t x = (uint32_t)w;
    do {
#pragma unroll
        for (int round = 3; round >= 0; --round) {
            x ^= x >> f.shift;
            x = ((x - f.add[round]) * f.inv[round]) & f.mask;
        }
    } while (x >= f.nw);
    return (int)x;
}

// draws of slot j of the half-step to accept: walker and log(u); of the half-step to propose: walker, partner, z and (P - 1) log z
// (emcee moves/red_blue.py, moves/stretch.py: z ~ g(z) on [1/a, a], partner from the complementary half).  S: what a step kernel knows of its two half-steps --
// it_acc, half_acc, split_acc; it_prop, half_prop, split_prop; the key k0, k1; a; P.
template <class S>
__device__ __forceinline__ void dl_ens_draw_accept(const S& s, int j, int half, int& i, double& logu) {
#pragma clang fp contract(off)
    i = dl_ens_split_at(s.split_acc, s.half_acc * half + j);
    const DlPhilox r = dl_philox4x32((uint32_t)s.it_acc, (uint32_t)((unsigned long long)s.it_acc >> 32), (uint32_t)j, DL_ENS_STREAM_ACCEPT + s.half_acc, s.k0, s.k1);
    logu = log(dl_uniform53(r.x[0], r.x[1]));
}

template <class S>
__device__ __forceinline__ void dl_ens_draw_move(const S& s, int j, int half, int& is, int& ic, double& zz, double& factor) {
#pragma clang fp contract(off)
    const DlPhilox r = dl_philox4x32((uint32_t)s.it_prop, (uint32_t)((unsigned long long)s.it_prop >> 32), (uint32_t)j, DL_ENS_STREAM_MOVE + s.half_prop, s.k0, s.k1);
    const double u = dl_uniform53(r.x[0], r.x[1]);
    const double t = (s.a - 1.) * u + 1.;
    zz = (t * t) / s.a;
    factor = (s.P - 1.) * log(zz);
    ic = dl_ens_split_at(s.split_prop, (1 - s.half_prop) * half + (int)(r.x[2] % (uint32_t)half));
    is = dl_ens_split_at(s.split_prop, s.half_prop * half + j);
}

// asynchronous copy of n doubles (16-byte aligned source) into LDS: 16-byte LDS-DMA chunks (global_load_lds_dwordx4: no registers, nothing waits until the
// workgroup's barrier), lane l of a wavefront writes chunk l of the wavefront's 1 KB slot.  rot_c > 0: rows of rot_c chunks, chunk c of row r lands at position
// (c + r) % rot_c of the row (threads that walk their own row chunk by chunk then spread over the LDS banks instead of all hitting the same two).
__device__ __forceinline__ void dl_ens_stage(double* dst, const double* __restrict__ src, int n, int rot_c, int wave, int lane, int nthr) {
    const int chunks = n >> 1;
    for (int c0 = wave * 64; c0 < chunks; c0 += nthr) {
        const int slot = c0 + lane;
        if (slot < chunks) {
            int from = slot;
            if (rot_c > 0) { const int r = slot / rot_c, cp = slot - r * rot_c; int c = cp - r % rot_c; if (c < 0) c += rot_c; from = r * rot_c + c; }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 2 * (size_t)from), (__attribute__((address_space(3))) void*)(dst + 2 * (size_t)c0), 16, 0, 0);
        }
    }
    if ((n & 1) && wave == 0 && lane == 0) dst[n - 1] = src[n - 1];
}
