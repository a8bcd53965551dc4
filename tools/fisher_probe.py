"""Time one ``dl_eval_fisher_analytic`` call against one ``dl_eval_fisher`` call on the config-2 likelihood, in ONE process on one GPU: device events around each call,
after warm-up, median of ``reps`` calls.

    python tools/fisher_probe.py [B=1024] [reps=40] [analytic|finite|both] [parent_lib]

``parent_lib``: a ``libdesilike_amd.so`` built from the commit before the analytic entry point existed; its ``dl_eval_fisher`` is timed as well (the yardstick: a second
context of the same configuration bound to that library, in this process).  Under ``rocprofv3 --kernel-trace --stats -- python tools/fisher_probe.py 1024 40 analytic``
the kernel table is the breakdown of the analytic call."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def context_on_library(like, path):
    """A second device context of ``like`` bound to another build of the library (symbols that build lacks are left unbound).  ``Context`` takes the library from
    ``_lib.load()`` once, in its constructor, and keeps it in ``self._lib``: the module global is swapped for the duration of that constructor only, and the returned
    context goes on calling the OTHER CDLL (which it keeps alive) for all of its methods.  ``like``: a likelihood, or a configuration (dict; device 0).  Probe use only."""
    from desilike_amd import _lib
    current = _lib.load()
    other = ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib.SYMBOLS.items():
        if hasattr(other, name): getattr(other, name).restype, getattr(other, name).argtypes = restype, argtypes
    _lib._lib = other
    try:
        if isinstance(like, dict): return _lib.Context(like, device=0)
        return _lib.Context(like._spec({}, like._flatdata_list(), like._precision_input), device=like.device)
    finally:
        _lib._lib = current


def median_time(call, reps, warmup=10):
    import torch
    for _ in range(warmup): call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(); call(); stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e3)
    times = np.sort(times)
    return float(np.median(times)), float(times[len(times) // 10]), float(times[-1 - len(times) // 10])


def main():
    import torch
    from bench_configs import make_cfg2
    from desilike_amd.fisher import Fisher
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 40, 20)
    mode = sys.argv[3] if len(sys.argv) > 3 else 'both'
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    g, like = make_cfg2()
    fisher = Fisher(like)
    ctx = fisher._get_context()
    rng = np.random.RandomState(0)
    centers = np.array([[param.ref.sample(random_state=rng) for param in like.varied_params] for _ in range(B)])
    device = torch.device('cuda', ctx.device)
    c = torch.as_tensor(centers, device=device).contiguous()
    steps = torch.as_tensor(fisher.steps(centers), device=device).contiguous()
    P = c.shape[1]
    out = [torch.empty((B, P, P), dtype=torch.float64, device=device), torch.empty((B, P), dtype=torch.float64, device=device), torch.empty(B, dtype=torch.float64, device=device)]
    results = {}
    if mode in ('analytic', 'both'):
        results['analytic'] = median_time(lambda: ctx.eval_fisher_analytic(c, *out), reps)
    if mode in ('finite', 'both'):
        results['finite'] = median_time(lambda: ctx.eval_fisher(c, steps, *out), reps)
    if parent:
        pctx = context_on_library(like, parent)
        results['finite_parent'] = median_time(lambda: pctx.eval_fisher(c, steps, *out), reps)
        if 'analytic' in results: results['analytic_again'] = median_time(lambda: ctx.eval_fisher_analytic(c, *out), reps)   # (drift of the box over the run)
    for name, (median, p10, p90) in results.items():
        print('{:15s} B = {:d}  P = {:d}: median {:9.1f} us  (p10 {:.1f}, p90 {:.1f}; {:d} calls)'.format(name, B, P, median, p10, p90, reps))
    if 'analytic' in results:
        for name in ('finite', 'finite_parent'):
            if name in results: print('analytic / {} = {:.3f}'.format(name, results['analytic'][0] / results[name][0]))


if __name__ == '__main__':
    main()
