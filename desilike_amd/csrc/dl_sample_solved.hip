// dl_sample_solved.hip -- the draw kernel of dl_sample_solved (dl_sample_solved.h states the arithmetic and the random draws) and its launcher.
#include "dl_kernels.h"
#include "dl_sample_solved.h"

// ONE LANE PER POINT, as dl_finalize_marg_gram_kernel: the lane factorises the posterior precision of its point once and loops over the draws.  No LDS, no
// barrier, no cross-lane traffic; a wavefront per workgroup, so that the NS = 16 triangle (136 doubles) may use the whole register file of a lane.
template <int NS>
__global__ __launch_bounds__(64) void dl_sample_solved_kernel(DlMargDev mg, const double* __restrict__ hessian, const double* __restrict__ solved,
                                                               const double* __restrict__ loglike, const double* __restrict__ logprior,
                                                               const int32_t* __restrict__ status_in, int64_t B, int64_t index0, int size, uint32_t k0, uint32_t k1,
                                                               double* __restrict__ solved_out, double* __restrict__ loglike_out, double* __restrict__ logprior_out,
                                                               int32_t* __restrict__ status_out) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int st = dl_sample_solved_lane<NS>(hessian + (size_t)b * NS * NS, solved + (size_t)b * NS, mg, loglike[b], logprior[b], status_in[b], index0 + b, size, k0, k1,
                                             solved_out + (size_t)b * size * NS, loglike_out + (size_t)b * size, logprior_out + (size_t)b * size);
    if (status_out) status_out[b] = st;
}

void dl_launch_sample_solved(const DlMargDev& mg, const double* hessian, const double* solved, const double* loglike, const double* logprior, const int32_t* status_in,
                             int64_t B, int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out, double* logprior_out, int32_t* status_out,
                             hipStream_t stream) {
    if (B <= 0 || size <= 0) return;
    const unsigned grid = (unsigned)((B + 63) / 64);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    auto launch = [&](auto kernel) {
        DL_LAUNCH(kernel, dim3(grid), dim3(64), 0, stream, mg, hessian, solved, loglike, logprior, status_in, B, index0, size, k0, k1, solved_out, loglike_out, logprior_out,
                  status_out);
    };
    switch (mg.n_s) {
        case 1: launch(dl_sample_solved_kernel<1>); break;
        case 2: launch(dl_sample_solved_kernel<2>); break;
        case 3: launch(dl_sample_solved_kernel<3>); break;
        case 4: launch(dl_sample_solved_kernel<4>); break;
        case 5: launch(dl_sample_solved_kernel<5>); break;
        case 6: launch(dl_sample_solved_kernel<6>); break;
        case 7: launch(dl_sample_solved_kernel<7>); break;
        case 8: launch(dl_sample_solved_kernel<8>); break;
        case 9: launch(dl_sample_solved_kernel<9>); break;
        case 10: launch(dl_sample_solved_kernel<10>); break;
        case 11: launch(dl_sample_solved_kernel<11>); break;
        case 12: launch(dl_sample_solved_kernel<12>); break;
        case 13: launch(dl_sample_solved_kernel<13>); break;
        case 14: launch(dl_sample_solved_kernel<14>); break;
        case 15: launch(dl_sample_solved_kernel<15>); break;
        case 16: launch(dl_sample_solved_kernel<16>); break;
        default: break;   // (dl_create admits 1 .. DL_MAX_SOLVED solved parameters; dl_sample_solved returns before the launch when there is none)
    }
}
