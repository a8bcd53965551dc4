// dl_fd_gradient.hip -- the gradient route NUTS and MCLMC share (dl_sampler_dev.h, DlFdGradient): dl_eval_logposterior_grad where the context is in its scope;
// otherwise central differences: dl_fd_stencil_kernel writes the C (2 P + 1) rows q, q -+ step e_i (steps: Parameter.delta, shortened near a prior bound),
// dl_eval_logposterior evaluates them, dl_fd_diff_kernel forms log-posterior and gradient.
#include "dl_sampler_dev.h"

namespace {

// finite-difference stencil of the pending positions: row (c, 0) = q, (c, 1 + 2 i) = q - lower_i e_i, (c, 2 + 2 i) = q + upper_i e_i
__device__ inline void dl_fd_steps(const double* q, const double* delta, const double* limits, int i, double* lower, double* upper) {
    *lower = fmax(fmin(delta[2 * i], q[i] - limits[2 * i]), 0.);
    *upper = fmax(fmin(delta[2 * i + 1], limits[2 * i + 1] - q[i]), 0.);
}

__global__ void dl_fd_stencil_kernel(const double* qn, const double* delta, const double* limits, int C, int P, double* rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, R = 2 * P + 1;
    if (idx >= (long long)C * R * P) return;
    const int i = (int)(idx % P);
    const long long cr = idx / P;
    const int r = (int)(cr % R), c = (int)(cr / R);
    const double* q = qn + (size_t)c * P;
    double value = q[i];
    if (r > 0 && (r - 1) / 2 == i) {
        double lower, upper;
        dl_fd_steps(q, delta, limits, i, &lower, &upper);
        value = (r & 1) ? q[i] - lower : q[i] + upper;
    }
    rows[idx] = value;
}

__global__ void dl_fd_diff_kernel(const double* qn, const double* delta, const double* limits, const double* vals, int C, int P, double* lp, double* grad) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)C * P) return;
    const int i = (int)(idx % P), c = (int)(idx / P);
    const double* v = vals + (size_t)c * (2 * P + 1);
    double lower, upper;
    dl_fd_steps(qn + (size_t)c * P, delta, limits, i, &lower, &upper);
    grad[idx] = (v[2 + 2 * i] - v[1 + 2 * i]) / (lower + upper);     // (what a value that is not finite means is the sampler's step kernel's)
    if (i == 0) lp[c] = v[0];
}

}  // namespace

bool dl_fd_gradient_create(DlFdGradient* g, size_t C, size_t P, int mode, const double* fd_delta, const double* fd_limits) {
    const size_t nrow = C * (2 * P + 1);
    g->mode = mode; g->finite = mode == 2;
    bool ok = dl_dev_alloc(&g->lp, C) && dl_dev_alloc(&g->grad, C * P);
    if (ok && fd_delta && fd_limits)
        ok = dl_dev_alloc(&g->fd_rows, nrow * P) && dl_dev_alloc(&g->fd_vals, nrow) && dl_dev_alloc(&g->fd_delta, 2 * P) && dl_dev_alloc(&g->fd_limits, 2 * P) &&
             hipMemcpy(g->fd_delta, fd_delta, 2 * P * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(g->fd_limits, fd_limits, 2 * P * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    return ok;
}

void dl_fd_gradient_destroy(DlFdGradient* g) {
    dl_dev_free({(void**)&g->lp, (void**)&g->grad, (void**)&g->fd_rows, (void**)&g->fd_vals, (void**)&g->fd_delta, (void**)&g->fd_limits});
}

int dl_fd_gradient_eval(DlFdGradient* g, dl_ctx* ctx, const char* who, const double* q, int C, int P, hipStream_t stream) {
    if (!g->finite) {
        const int rc = dl_eval_logposterior_grad(ctx, q, C, g->lp, g->grad, nullptr, stream);
        if (rc == 1) return 1;
        if (rc == 0) return 0;
        if (g->mode == 1) return dl_fail(std::string(who) + ": the context is outside the analytic gradient's scope (use the finite-difference mode)");
        g->finite = true;
    }
    if (!g->fd_rows) return dl_fail(std::string(who) + ": central differences need the steps and limits given to " + who + "_create");
    const long long nrow = (long long)C * (2 * P + 1);
    hipLaunchKernelGGL(dl_fd_stencil_kernel, dim3((unsigned)((nrow * P + 255) / 256)), dim3(256), 0, stream, q, g->fd_delta, g->fd_limits, C, P, g->fd_rows);
    if (dl_eval_logposterior(ctx, g->fd_rows, nrow, g->fd_vals, nullptr, stream)) return 1;
    hipLaunchKernelGGL(dl_fd_diff_kernel, dim3((unsigned)(((long long)C * P + 255) / 256)), dim3(256), 0, stream, q, g->fd_delta, g->fd_limits, g->fd_vals, C, P,
                       g->lp, g->grad);
    return 0;
}
