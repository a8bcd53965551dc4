"""Time the data batch (csrc/dl_data_batch.h) on the cfg2 shape: python tools/data_batch_probe.py batch|single [--points 1024] [--vectors 1024]

batch:  ONE dl_eval_logposterior_data call, cross mode, points x vectors log-posteriors: median of 20 calls between HIP events on the stream, and the kernels' own
        intervals from the events on their dispatch packets (dl_profile_*): theory, window GEMM, the cross kernel.
single: what the same table costs without a data batch: `vectors` separate dl_eval_logposterior calls of `points` points (on ONE context: the per-mock context
        creation -- Cholesky factor, whitening of the window, upload -- is timed separately and reported per context).  Runs on any build of the library
        (DL_LIB_PATH=<the parent's>).
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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('mode', choices=['batch', 'single'])
    parser.add_argument('--points', type=int, default=1024)
    parser.add_argument('--vectors', type=int, default=1024)
    args = parser.parse_args()
    import torch
    from golden_utils import load_golden, spec_from_golden
    from desilike_amd._lib import Context
    g = load_golden('cfg2_shapefit_window')
    spec = spec_from_golden(g)
    rng = np.random.RandomState(1)
    rows = np.asarray(g['theta'], dtype='f8')
    rows = rows[((rows >= g['priors'][:, 1]) & (rows <= g['priors'][:, 2])).all(axis=1)]
    a = rng.uniform(size=(args.points, 1))
    theta = a * rows[rng.randint(len(rows), size=args.points)] + (1. - a) * rows[rng.randint(len(rows), size=args.points)]
    flatdata = np.ravel(spec['observables'][0]['flatdata'])
    mocks = flatdata + 0.05 * np.abs(flatdata) * rng.standard_normal((args.vectors, flatdata.size))
    device = torch.device('cuda', 0)
    th = torch.as_tensor(theta, device=device).contiguous()
    t0 = time.perf_counter()
    ctx = Context(spec, device=0)
    create_ms = 1e3 * (time.perf_counter() - t0)      # (includes the first use of the device by this process)
    t0 = time.perf_counter()
    Context(spec, device=0).close()
    create_ms = min(create_ms, 1e3 * (time.perf_counter() - t0))
    result = dict(mode=args.mode, points=args.points, vectors=args.vectors, context_create_ms=create_ms)
    if args.mode == 'batch':
        t0 = time.perf_counter()
        ctx.set_data_batch(mocks)
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
        ctx.profile_enable(1)
        for _ in range(20): ctx.eval_logposterior_data(th, out=out)
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        result['kernels_us'] = {key: 1e3 * float(prof[key]) for key in ['theory', 'window_gemm', 'finalize']}
        result['cross_kernel_share_of_kernels'] = result['kernels_us']['finalize'] / sum(result['kernels_us'].values())
        result['cross_kernel_share_of_call'] = result['kernels_us']['finalize'] / result['call_us']
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
    print(json.dumps(result))


if __name__ == '__main__':
    main()
