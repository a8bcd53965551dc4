"""Time ``dl_sample_solved_data`` (csrc/dl_sample_solved_data.h) against ``dl_eval_solved_data`` and against the route that exists without it, in ONE process on one GPU:
device events around each call, 10 warm-up calls, median of ``reps`` calls.

    python tools/sample_solved_data_probe.py time|trace|single --shape cfg3|eft [--points 65536] [--vectors 64] [--reps 40] [--parent-lib PATH]

shape cfg3: the benchmarked emulated shape (stacked layout, 5 marginalised parameters); eft: tests/marg_counts_cases.py build(120, 12) (tools/data_batch_marg_probe.py).
time:   ``points`` rows against ``vectors`` mocks (row b against mock b % vectors): dl_eval_solved_data, dl_sample_solved_data at size 1 and 4, and -- with
        ``--parent-lib``, a libdesilike_amd.so built from the commit before the entry point existed -- dl_eval_solved_data of that library on a second context.
trace:  size = 1 calls only: under ``rocprofv3 --kernel-trace --stats -- python tools/sample_solved_data_probe.py trace ...`` the row of dl_dbm_draw_kernel is the draw
        kernel's own time.
single: the same chains through ``vectors`` per-mock contexts and dl_sample_solved (points / vectors rows each): context creation and calls stated apart.
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('mode', choices=['time', 'trace', 'single'])
    parser.add_argument('--shape', choices=['cfg3', 'eft'], default='cfg3')
    parser.add_argument('--points', type=int, default=65536)
    parser.add_argument('--vectors', type=int, default=64)
    parser.add_argument('--reps', type=int, default=40)
    parser.add_argument('--parent-lib', default=None)
    args = parser.parse_args()
    import torch
    from desilike_amd._lib import Context
    from data_batch_marg_probe import shape
    from fisher_probe import context_on_library, median_time
    B, M = args.points, args.vectors
    spec, theta, mocks = shape(args.shape, B, M, False)
    device = torch.device('cuda', 0)
    th = torch.as_tensor(theta, device=device).contiguous()
    index = torch.as_tensor((np.arange(B) % M).astype('i4'), device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    ctx = Context(spec, device=0)
    ns = ctx.n_solved
    result = dict(mode=args.mode, shape=args.shape, points=B, vectors=M, n_data=ctx.n_data, n_solved=ns, reps=args.reps)
    status = torch.empty(B, dtype=torch.int32, device=device)

    def sampler(size):
        x = torch.empty((B, size, ns), dtype=torch.float64, device=device)
        ll, lp = torch.empty((B, size), dtype=torch.float64, device=device), torch.empty((B, size), dtype=torch.float64, device=device)

        def call():
            rc = ctx._lib.dl_sample_solved_data(ctx._handle, ctypes.c_void_p(th.data_ptr()), B, ctypes.c_void_p(index.data_ptr()), 0, size, 42, ctypes.c_void_p(x.data_ptr()),
                                                ctypes.c_void_p(ll.data_ptr()), ctypes.c_void_p(lp.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream))
            assert rc == 0
        return call

    def solved(context):
        out, sol = torch.empty(B, dtype=torch.float64, device=device), torch.empty((B, ns), dtype=torch.float64, device=device)
        return lambda: context.eval_solved_data(th, index, out=out, status=status, solved=sol, stream=stream)

    if args.mode in ('time', 'trace'):
        ctx.set_data_batch(mocks, solved=True)
        if args.mode == 'trace':
            result['sample_size1_us'] = median_time(sampler(1), args.reps)
        else:
            result['eval_solved_data_us'] = median_time(solved(ctx), args.reps)
            result['sample_size1_us'] = median_time(sampler(1), args.reps)
            result['sample_size4_us'] = median_time(sampler(4), args.reps)
            if args.parent_lib:
                parent = context_on_library(spec, args.parent_lib)
                parent.set_data_batch(mocks, solved=True)
                result['eval_solved_data_parent_us'] = median_time(solved(parent), args.reps)
            result['eval_solved_data_again_us'] = median_time(solved(ctx), args.reps)      # (drift of the box over the run)
            yardstick = result.get('eval_solved_data_parent_us', result['eval_solved_data_us'])[0]
            result['ratio_size1'], result['ratio_size4'] = result['sample_size1_us'][0] / yardstick, result['sample_size4_us'][0] / yardstick
            result['finite'] = float((status == 0).double().mean())
    else:
        import data_batch_utils as dbu
        per = B // M
        t0 = time.perf_counter()
        if args.shape == 'cfg3':
            case = dbu.get_case('boundary_cfg3_stacked_bench')
            contexts = [Context(case.spec_with_data(mock), device=0) for mock in mocks]
        else:
            from test_gpu_data_batch_marg import with_data
            sizes = [np.size(obs['flatdata']) for obs in spec['observables']]
            contexts = [Context(with_data(spec, sizes, mock), device=0) for mock in mocks]
        torch.cuda.synchronize()
        result['contexts_total_ms'] = 1e3 * (time.perf_counter() - t0)
        result['context_create_ms'] = result['contexts_total_ms'] / M
        chunks = [th[m * per:(m + 1) * per].contiguous() for m in range(M)]
        for size in (1, 4):
            for context, chunk in zip(contexts[:4], chunks): context.sample_solved(chunk, index0=0, size=size, seed=42)      # warm-up: workspaces of the shape
            torch.cuda.synchronize()
            times = []
            for _ in range(5):
                t0 = time.perf_counter()
                for m, (context, chunk) in enumerate(zip(contexts, chunks)): context.sample_solved(chunk, index0=m * per, size=size, seed=42)
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            result['calls_size{:d}_ms'.format(size)] = float(np.median(times))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
