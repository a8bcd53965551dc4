// dl_sampler_dev.h -- what the translation units of the device-resident samplers share (dl_nuts / dl_mclmc / dl_smc / dl_nested / dl_mh / dl_ensemble .hip): the
// lane-per-component layout and the workgroup reductions their algorithm headers are instantiated with, the population's moments and Cholesky bodies, the gradient
// with its central-difference fallback (dl_fd_gradient.hip), error reporting and device allocation.  For hipcc only: the algorithm headers (dl_*.h) stay free of HIP
// and never include this file.  A new sampler starts from here.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "../../include/desilike_amd.h"
#include "dl_kernels.h"   // dl_set_last_error
#include "dl_smc.h"       // dl_smc_moment_partial, dl_smc_factor; dl_nuts.h

// ---- errors -----------------------------------------------------------------------------------------------------------------------------------------------------
inline int dl_fail(const std::string& msg) {
    dl_set_last_error(msg.c_str());
    return 1;
}

#define DL_HIP_CHECK(call)                                                                               \
    do {                                                                                                 \
        hipError_t err__ = (call);                                                                       \
        if (err__ != hipSuccess) return dl_fail(std::string(#call) + ": " + hipGetErrorString(err__));   \
    } while (0)

// ---- device arrays ----------------------------------------------------------------------------------------------------------------------------------------------
// n zeroed elements
template <class T>
bool dl_dev_alloc(T** p, size_t n) {
    return hipMalloc((void**)p, n * sizeof(T)) == hipSuccess && hipMemset(*p, 0, n * sizeof(T)) == hipSuccess;
}

inline void dl_dev_free(std::initializer_list<void**> ptrs) {
    for (void** p : ptrs)
        if (*p) { (void)hipFree(*p); *p = nullptr; }
}

// ---- layouts ----------------------------------------------------------------------------------------------------------------------------------------------------
// the device's component layout: lane = component (a wavefront per chain, particle or point)
struct DlWave {
    static constexpr int W = 1;
    int P, lane;
    __device__ int comp(int) const { return lane; }
    __device__ bool on(int) const { return lane < P; }
    __device__ double sum(const double* x) const {
        double v = x[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    }
    __device__ double at(const double* x, int k) const { return __shfl(x[0], k, 64); }
    __device__ void sync() const { __syncthreads(); }      // (the Cholesky kernels' workgroup is one wavefront)
};

// the n threads of a workgroup: a wavefront's butterfly, then the wavefronts in index order
struct DlBlock {
    int tid, n;
    double* red;      // [2 * wavefronts] LDS
    __device__ void sum2(double& a, double& b) const {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
        const int nw = n >> 6;
        __syncthreads();      // (the previous reduction's reads)
        if ((tid & 63) == 0) { red[2 * (tid >> 6)] = a; red[2 * (tid >> 6) + 1] = b; }
        __syncthreads();
        a = 0.; b = 0.;
        for (int w = 0; w < nw; ++w) { a += red[2 * w]; b += red[2 * w + 1]; }
    }
    __device__ double max(double v) const {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        const int nw = n >> 6;
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        v = red[0];
        for (int w = 1; w < nw; ++w) v = fmax(v, red[w]);
        return v;
    }
};

// ---- a population's moments and factor --------------------------------------------------------------------------------------------------------------------------
// a workgroup of DL_SMC_MOMENT_WAVES wavefronts: the mean of the N points x [N, P] of weights W of population k, then the lower triangle of row `row` of their
// covariance into a.cov [K, P, P], wavefront partials added in index order; row 0 also writes a.mean [K, P].  (a: the kernel's arguments, DlSmcArgs or DlNestedArgs,
// by reference: the two pointers are read where they are used, after the sums, as before the bodies were shared -- passed by value they cost two more SGPRs)
template <class A>
__device__ __forceinline__ void dl_pop_moments_row(const A& a, const double* x, const double* W, int N, int k, int row) {
    __shared__ double part[DL_SMC_MOMENT_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, P = a.P;
    const DlWave l{P, lane};
    DlNutsVec<DlWave> m, acc;
    m.x[0] = 0.;
    dl_smc_moment_partial(l, x, W, N, w, DL_SMC_MOMENT_WAVES, -1, m, 0., acc);
    part[w][lane] = acc.x[0];
    __syncthreads();
    double s = 0.;
    for (int v = 0; v < DL_SMC_MOMENT_WAVES; ++v) s += part[v][lane];
    m.x[0] = s;
    const double mrow = __shfl(s, row, 64);
    __syncthreads();
    dl_smc_moment_partial(l, x, W, N, w, DL_SMC_MOMENT_WAVES, row, m, mrow, acc);
    part[w][lane] = acc.x[0];
    __syncthreads();
    if (w == 0 && lane < P) {
        s = 0.;
        for (int v = 0; v < DL_SMC_MOMENT_WAVES; ++v) s += part[v][lane];
        if (lane <= row) a.cov[((size_t)k * P + row) * P + lane] = s;
        if (row == 0) a.mean[(size_t)k * P + lane] = x[lane] + m.x[0];
    }
}

// a workgroup of one wavefront: the factor of cov [P, P] (or its diagonal fallback from the priors' widths) into out [P, P]
__device__ __forceinline__ void dl_pop_cholesky(int P, const double* cov, const double* widths, double* out) {
    __shared__ double C[DL_SMC_MAX_P * DL_SMC_MAX_P];
    const int lane = threadIdx.x;
    const DlWave l{P, lane};
    for (int e = lane; e < P * P; e += 64) C[e] = 0.;
    __syncthreads();
    dl_smc_factor(l, cov, widths, C);
    for (int e = lane; e < P * P; e += 64) out[e] = C[e];
}

// ---- the gradient of NUTS and MCLMC (dl_fd_gradient.hip) --------------------------------------------------------------------------------------------------------
struct DlFdGradient {
    int mode = 0;             // 0 auto, 1 analytic, 2 finite
    bool finite = false;
    double *lp = nullptr, *grad = nullptr;      // [C], [C, P]: the results
    double *fd_rows = nullptr, *fd_vals = nullptr, *fd_delta = nullptr, *fd_limits = nullptr;
};

// the arrays for C rows of P parameters (the central-difference ones where both fd_delta [P, 2] and fd_limits [P, 2] are given); false: a device allocation failed
bool dl_fd_gradient_create(DlFdGradient* g, size_t C, size_t P, int mode, const double* fd_delta, const double* fd_limits);
void dl_fd_gradient_destroy(DlFdGradient* g);
// log-posterior [C] and gradient [C, P] of rows q [C, P] into g->lp / g->grad: analytic where the context is in its scope, else (once and for all) central differences
int dl_fd_gradient_eval(DlFdGradient* g, dl_ctx* ctx, const char* who, const double* q, int C, int P, hipStream_t stream);
