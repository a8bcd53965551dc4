"""Time ``dl_sample_solved`` against ``dl_eval_batch_derived`` on the marginalised config-3 likelihood (tests/test_host_api.py::make_cfg3(marg=True): the feature-Gram
tail, 5 solved parameters), in ONE process on one GPU: device events around each call, 10 warm-up calls, median of ``reps`` calls.

    python tools/sample_solved_probe.py [B=65536] [reps=40] [time|trace] [parent_lib]

``parent_lib``: a ``libdesilike_amd.so`` built from the commit before the entry point existed; its ``dl_eval_batch_derived`` is the yardstick (a second context of the
same configuration bound to that library, in this process).  ``trace``: ``size = 1`` calls only -- under ``rocprofv3 --kernel-trace --stats -- python
tools/sample_solved_probe.py 65536 40 trace`` the kernel table is the breakdown of the call and the row of ``dl_sample_solved_kernel`` the draw kernel's own time."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    import torch
    from fisher_probe import context_on_library, median_time
    from test_host_api import make_cfg3
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 40, 20)
    mode = sys.argv[3] if len(sys.argv) > 3 else 'time'
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    g, like = make_cfg3(marg=True)
    ctx = like._get_context()
    ns = ctx.n_solved
    rng = np.random.RandomState(0)
    theta = np.column_stack([np.clip(param.ref.sample(size=B, random_state=rng), *param.prior.limits) for param in like.varied_params])
    device = torch.device('cuda', ctx.device)
    th = torch.as_tensor(theta, dtype=torch.float64, device=device).contiguous()
    stream = torch.cuda.current_stream(device).cuda_stream
    status = torch.empty(B, dtype=torch.int32, device=device)

    def sampler(size):
        x = torch.empty((B, size, ns), dtype=torch.float64, device=device)
        ll, lp = torch.empty((B, size), dtype=torch.float64, device=device), torch.empty((B, size), dtype=torch.float64, device=device)

        def call():
            rc = ctx._lib.dl_sample_solved(ctx._handle, ctypes.c_void_p(th.data_ptr()), B, 0, size, 42, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(ll.data_ptr()),
                                           ctypes.c_void_p(lp.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream))
            assert rc == 0
        return call

    def derived(context):
        out = dict(loglike=torch.empty(B, dtype=torch.float64, device=device), logprior=torch.empty(B, dtype=torch.float64, device=device), status=status,
                   solved=torch.empty((B, ns), dtype=torch.float64, device=device), hessian=torch.empty((B, ns, ns), dtype=torch.float64, device=device))
        return lambda: context.eval_batch_derived(th, stream=stream, **out)

    results = {}
    if mode == 'trace':
        results['sample size=1'] = median_time(sampler(1), reps)
    else:
        results['derived'] = median_time(derived(ctx), reps)
        results['sample size=1'] = median_time(sampler(1), reps)
        results['sample size=4'] = median_time(sampler(4), reps)
        if parent:
            results['derived_parent'] = median_time(derived(context_on_library(like, parent)), reps)
        results['derived_again'] = median_time(derived(ctx), reps)   # (drift of the box over the run)
    for name, (median, p10, p90) in results.items():
        print('{:15s} B = {:d}  n_solved = {:d}: median {:9.1f} us  (p10 {:.1f}, p90 {:.1f}; {:d} calls)'.format(name, B, ns, median, p10, p90, reps))
    for name in ('derived', 'derived_parent'):
        for size in (1, 4):
            if name in results and 'sample size={:d}'.format(size) in results:
                print('sample size={:d} / {} = {:.3f}'.format(size, name, results['sample size={:d}'.format(size)][0] / results[name][0]))


if __name__ == '__main__':
    main()
