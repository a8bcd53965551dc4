"""Time the data batch of a context with analytically solved parameters (csrc/dl_data_batch_marg.h):
    python tools/data_batch_marg_probe.py batch|single|plain --shape cfg3|eft [--points 1024] [--vectors 1024]

shape cfg3: the benchmarked emulated shape (stacked layout, 5 marginalised parameters: tests/golden boundary_cfg3_stacked_bench); eft: tests/marg_counts_cases.py build(120, 12)
            (two EFT-like Kaiser tracers, 12 solved parameters of which 6 have point-dependent rows).
batch:  ONE dl_eval_logposterior_data call, cross mode, points x vectors log-posteriors: median of 20 calls between HIP events on the stream, and the kernels' own
        intervals from the events on their dispatch packets (dl_profile_*): theory, GEMM, and the LAST launch of the finalize phase, the pair kernel (the point
        kernel before it is what is left of the call).
single: the route that exists without it: `vectors` dl_eval_logposterior calls of `points` points on ONE solved context, and the time to create one per-mock context.
plain:  (eft only) as a scale, the existing dl_data_cross_kernel at the same n: the same likelihood with its solved parameters fixed, one cross call.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def shape(name, points, vectors, plain):
    rng = np.random.RandomState(1)
    if name == 'cfg3':
        import data_batch_utils as dbu
        case = dbu.get_case('boundary_cfg3_stacked_bench')
        spec, flatdata, theta = case.spec, case.flatdata, case.points(points)
        covariance = np.linalg.inv(case.precision if case.precision.ndim == 2 else np.diag(case.precision))
    else:
        import marg_counts_cases as mc
        case = mc.get_case(120, 12)
        like = case.likelihood(np.ones(12, dtype='?'))
        like.initialize()
        spec = like._spec({}, like._flatdata_list(), like._precision_input, drop_solved=plain)
        flatdata, covariance = case.flatdata, case.covariance
        a = rng.uniform(size=(points, 1))
        theta = a * case.theta[rng.randint(len(case.theta), size=points)] + (1. - a) * case.theta[rng.randint(len(case.theta), size=points)]
    mocks = flatdata + rng.multivariate_normal(np.zeros(flatdata.size), covariance, size=vectors)
    return spec, np.ascontiguousarray(theta), mocks


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('mode', choices=['batch', 'single', 'plain'])
    parser.add_argument('--shape', choices=['cfg3', 'eft'], default='cfg3')
    parser.add_argument('--points', type=int, default=1024)
    parser.add_argument('--vectors', type=int, default=1024)
    args = parser.parse_args()
    import torch
    from desilike_amd._lib import Context
    spec, theta, mocks = shape(args.shape, args.points, args.vectors, args.mode == 'plain')
    device = torch.device('cuda', 0)
    th = torch.as_tensor(theta, device=device).contiguous()
    ctx = Context(spec, device=0)
    t0 = time.perf_counter()
    Context(spec, device=0).close()
    create_ms = 1e3 * (time.perf_counter() - t0)
    result = dict(mode=args.mode, shape=args.shape, points=args.points, vectors=args.vectors, n_data=ctx.n_data, n_solved=ctx.n_solved, context_create_ms=create_ms)
    if args.mode in ('batch', 'plain'):
        t0 = time.perf_counter()
        ctx.set_data_batch(mocks, solved=args.mode == 'batch')
        result['data_set_ms'] = 1e3 * (time.perf_counter() - t0)
        out = torch.empty((args.points, args.vectors), dtype=torch.float64, device=device)
        for _ in range(5): ctx.eval_logposterior_data(th, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(); ctx.eval_logposterior_data(th, out=out); stop.record()
            torch.cuda.synchronize()
            times.append(1e3 * start.elapsed_time(stop))
        result['call_us'] = float(np.median(times)); result['call_us_min_max'] = [float(min(times)), float(max(times))]
        result['finite'] = float(torch.isfinite(out).double().mean())
        ctx.profile_enable(1)
        for _ in range(20): ctx.eval_logposterior_data(th, out=out)
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        result['kernels_us'] = {key: 1e3 * float(prof[key]) for key in ['theory', 'window_gemm', 'finalize']}
    else:
        out = torch.empty(args.points, dtype=torch.float64, device=device)
        for _ in range(20): ctx.eval_logposterior(th, out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.vectors): ctx.eval_logposterior(th, out)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        result['calls_total_us'] = 1e6 * total
        result['per_call_us'] = 1e6 * total / args.vectors
        result['contexts_total_ms'] = create_ms * args.vectors
    print(json.dumps(result))


if __name__ == '__main__':
    main()
