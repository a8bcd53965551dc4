"""Time ``dl_eval_fisher_analytic_data`` against its neighbours on the config-2 likelihood with a data batch, in ONE process on one GPU: device events around each
call, after warm-up, median of ``reps`` calls, the variants INTERLEAVED in blocks of ten calls so that a drift of the box lands on all of them (the
method of tools/fisher_probe.py).

    python tools/data_analytic_probe.py [B=1024] [reps=40] [all|analytic_data|grad_data] [parent_lib]

``B`` centres against ``M = min(B, 1024)`` data vectors, ``index = b mod M``.  Variants: ``analytic_data`` (dl_eval_fisher_analytic_data), ``analytic``
(dl_eval_fisher_analytic at the same centres), ``finite_data`` (dl_eval_fisher_data of this tree), ``grad_data`` / ``grad`` (dl_eval_logposterior_grad_data and its
twin), ``logposterior_data``; ``parent_lib``: a ``libdesilike_amd.so`` built from the commit before the entry points existed -- its ``dl_eval_fisher_data`` is timed as
``finite_data_parent`` (a second context of the same configuration bound to that library, in this process).  A single variant
(``analytic_data`` / ``grad_data``) is the one to run under ``rocprofv3 --kernel-trace --stats -- python tools/data_analytic_probe.py 1024 40 analytic_data``: the
kernel table is the breakdown of that call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def interleaved(calls, reps, warmup=10, block=10):
    """{name: (median, p10, p90)} in microseconds: ``warmup`` calls of every variant, then blocks of ``block`` timed calls of each variant in turn until ``reps``."""
    import torch
    for call in calls.values():
        for _ in range(warmup): call()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    done = 0
    while done < reps:
        n = min(block, reps - done)
        for name, call in calls.items():
            for _ in range(n):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(); call(); stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) * 1e3)
        done += n
    out = {}
    for name, values in times.items():
        values = np.sort(values)
        out[name] = (float(np.median(values)), float(values[len(values) // 10]), float(values[-1 - len(values) // 10]))
    return out


def main():
    import torch
    from bench_configs import make_cfg2
    from desilike_amd._lib import Context
    from desilike_amd.fisher import Fisher
    from fisher_probe import context_on_library
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 40, 20)
    mode = sys.argv[3] if len(sys.argv) > 3 else 'all'
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    g, like = make_cfg2()
    fisher = Fisher(like)
    like.initialize()
    spec = like._spec({}, like._flatdata_list(), like._precision_input)
    ctx = Context(spec, device=like.device)
    rng = np.random.RandomState(0)
    centers = np.array([[param.ref.sample(random_state=rng) for param in like.varied_params] for _ in range(B)])
    M = min(B, 1024)
    flatdata = np.concatenate(like._flatdata_list())
    mocks = flatdata + 0.05 * np.abs(flatdata) * rng.standard_normal((M, flatdata.size))
    ctx.set_data_batch(mocks)
    device = torch.device('cuda', ctx.device)
    c = torch.as_tensor(centers, device=device).contiguous()
    index = torch.as_tensor((np.arange(B) % M).astype('i4'), device=device)
    steps = torch.as_tensor(fisher.steps(centers), device=device).contiguous()
    P = c.shape[1]
    out = [torch.empty((B, P, P), dtype=torch.float64, device=device), torch.empty((B, P), dtype=torch.float64, device=device), torch.empty(B, dtype=torch.float64, device=device)]
    lp, grad = torch.empty(B, dtype=torch.float64, device=device), torch.empty((B, P), dtype=torch.float64, device=device)
    calls = {}
    if mode in ('all', 'analytic_data'): calls['analytic_data'] = lambda: ctx.eval_fisher_analytic_data(c, index, *out)
    if mode == 'all':
        calls['analytic'] = lambda: ctx.eval_fisher_analytic(c, *out)
        calls['finite_data'] = lambda: ctx.eval_fisher_data(c, steps, index, *out)
    if parent:
        pctx = context_on_library(spec, parent)
        pctx.set_data_batch(mocks)
        calls['finite_data_parent'] = lambda: pctx.eval_fisher_data(c, steps, index, *out)
    if mode in ('all', 'grad_data'): calls['grad_data'] = lambda: ctx.eval_logposterior_grad_data(c, index, lp, grad)
    if mode == 'all':
        calls['grad'] = lambda: ctx.eval_logposterior_grad(c, lp, grad)
        calls['logposterior_data'] = lambda: ctx.eval_logposterior_data(c, index=index, out=lp)
    results = interleaved(calls, reps)
    for name, (median, p10, p90) in results.items():
        print('{:20s} B = {:d}  M = {:d}  P = {:d}: median {:9.1f} us  (p10 {:.1f}, p90 {:.1f}; {:d} calls)'.format(name, B, M, P, median, p10, p90, reps))
    if 'analytic_data' in results:
        for name in ('finite_data_parent', 'finite_data', 'analytic'):
            if name in results: print('analytic_data / {} = {:.3f}'.format(name, results['analytic_data'][0] / results[name][0]))
    if 'grad_data' in results and 'grad' in results: print('grad_data / grad = {:.3f}'.format(results['grad_data'][0] / results['grad'][0]))
    print('residual kernel: N_pad = {:d}, K_pad = {:d}; bytes = (n_slabs + 2) x B x N_pad x 8 with n_slabs the split of the tiled window GEMM at B rows'.format(ctx.info('N_pad'), ctx.info('K_pad')))


if __name__ == '__main__':
    main()
