"""GPU: the device-resident microcanonical Langevin sampler (dl_mclmc_*, desilike_amd/mclmc.py _DeviceMCLMC) against the NumPy statement of the same stage machine
(_HostMCLMC) fed by the same device gradient, its repeatability, its controller, its posterior, its state and errors."""
import functools

import numpy as np
import pytest

from test_host_api import make_cfg2, make_cfg5

pytestmark = pytest.mark.gpu
INTEGRATORS = ['isokinetic_leapfrog', 'isokinetic_mclachlan']


def _cfg5():
    g, like = make_cfg5()
    like.all_params = {'*.sn0': {'derived': '.marg'}}
    return like


def _start_near_a_bound(sampler, nchains, seed=0):
    """Chains at the parameters' values (jittered by a hundredth of the proposal scale), the first bounded parameter within 2 % of its prior's width of the upper bound."""
    rng = np.random.RandomState(seed)
    limits = sampler._fd_tables()[1]
    start = np.array([param.value for param in sampler.varied_params]) + 0.01 * sampler.scale * rng.standard_normal((nchains, len(sampler.scale)))
    bounded = [i for i in range(limits.shape[0]) if np.all(np.isfinite(limits[i]))][0]
    start[:, bounded] = limits[bounded, 1] - 0.02 * (limits[bounded, 1] - limits[bounded, 0]) * rng.uniform(0.05, 1., nchains)
    return start


def _engines(like, nchains, fac, step, L, integrator='isokinetic_mclachlan', gradient='auto', seed=5):
    """(_DeviceMCLMC, _HostMCLMC) on the same chains; the host's gradient is the context's own on the same rows (analytic, or central differences through
    dl_eval_logposterior on the stencil the device builds)."""
    import torch
    from desilike_amd.mclmc import MCLMCSampler, _DeviceMCLMC, _HostMCLMC
    sampler = MCLMCSampler(like, chains=nchains, adaptation=False, gradient=gradient, seed=seed)
    ctx, offset = like._get_posterior_context()
    delta, limits = sampler._fd_tables()
    ids = np.arange(nchains)
    dev = _DeviceMCLMC(ctx, offset, ids, integrator, seed, gradient, delta, limits)

    def f(q):
        t = torch.as_tensor(np.ascontiguousarray(q), device='cuda:{:d}'.format(ctx.device))
        if gradient != 'finite':
            out = ctx.eval_logposterior_grad(t)
            return out[0].cpu().numpy(), out[1].cpu().numpy()
        C, P = q.shape
        lower = np.maximum(np.minimum(delta[:, 0], q - limits[:, 0]), 0.)
        upper = np.maximum(np.minimum(delta[:, 1], limits[:, 1] - q), 0.)
        rows = np.repeat(q[:, None, :], 2 * P + 1, axis=1)
        index = np.arange(P)
        rows[:, 1 + 2 * index, index] = q - lower
        rows[:, 2 + 2 * index, index] = q + upper
        values = torch.empty(C * (2 * P + 1), dtype=torch.float64, device=t.device)
        ctx.eval_logposterior(torch.as_tensor(rows.reshape(-1, P), device=t.device).contiguous(), values)
        values = values.cpu().numpy().reshape(C, 2 * P + 1)
        with np.errstate(invalid='ignore', divide='ignore'):
            return values[:, 0], (values[:, 2::2] - values[:, 1::2]) / (lower + upper)

    host = _HostMCLMC(f, nchains, len(like.varied_params), chain_ids=ids, integrator=integrator, seed=seed, offset=offset)
    start = _start_near_a_bound(sampler, nchains)
    for engine in (dev, host):
        engine.set_preconditioner(fac)
        engine.set_hyper(step, L)
        engine.set_state(start)
    return dev, host, sampler


@functools.lru_cache(maxsize=None)
def _warm(config):
    """Hyper-parameters from a short warm-up on the device: (diagonal, dense preconditioner in the parameters' coordinates, step size, L)."""
    from desilike_amd.samplers import MCLMCSampler
    like = make_cfg2()[1] if config == 'cfg2' else _cfg5()
    s = MCLMCSampler(like, chains=32, seed=11, adaptation={'niterations': 300, 'dense_preconditioning': True}, gradient='auto' if config == 'cfg2' else 'finite')
    assert s.device_resident
    s.run(check_every=10, max_iterations=10)
    dense = s.scale[:, None] * s.hyp['factor']
    return np.sqrt(np.diag(dense @ dense.T)), dense, s.hyp['step_size'], s.hyp['L']


def _compare(dev, host, nsteps, chunk=16):
    from desilike_amd.mclmc import run_batch
    cd, ld, idv = run_batch(dev, nsteps, chunk=chunk)
    ch, lh, ih = run_batch(host, nsteps, chunk=chunk)
    assert np.array_equal(idv[..., 1], ih[..., 1]), 'the flags of the undone steps differ'
    assert np.allclose(ld, lh, rtol=1e-10, atol=1e-8), float(np.max(np.abs(ld - lh)))
    assert np.allclose(cd, ch, rtol=1e-10, atol=1e-8), float(np.max(np.abs(cd - ch)))
    assert np.allclose(idv[..., 2], ih[..., 2], rtol=1e-10, atol=0.)
    return idv


@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('integrator', INTEGRATORS)
def test_device_equals_the_host_statement(integrator, dense):
    diag, full, step, L = _warm('cfg2')
    dev, host, _ = _engines(make_cfg2()[1], 64, full if dense else diag, step, L, integrator=integrator)
    info = _compare(dev, host, 50)
    assert 0 < info[..., 1].sum() < info[..., 1].size        # the chains start next to a prior bound: some steps are undone
    assert dev.mclmc.info('gradients_per_step') == 1 + INTEGRATORS.index(integrator) and dev.mclmc.info('dense') == int(dense) and dev.steps == 50


def test_finite_difference_route_equals_the_host_statement():
    """Central differences (gradient='finite') on a marginalised likelihood (the constant of the marginalisation travels as the offset): the device differentiates
    through dl_eval_logposterior on its stencil."""
    diag, _, step, L = _warm('cfg5')
    dev, host, _ = _engines(_cfg5(), 32, diag, step, L, gradient='finite')
    _compare(dev, host, 40)
    assert dev.mclmc.info('finite') == 1


def test_repeatability_and_chunking():
    from desilike_amd.mclmc import run_batch
    diag, _, step, L = _warm('cfg2')
    runs = []
    for chunk in (40, 40, 10):
        dev, _, _ = _engines(make_cfg2()[1], 64, diag, step, L)
        runs.append(run_batch(dev, 40, chunk=chunk) + tuple(dev.get_state()))
    for other in runs[1:]:
        for x, y in zip(runs[0], other): assert np.array_equal(x, y)


def test_controller_on_the_device():
    from desilike_amd.mclmc import run_batch
    diag, _, step, L = _warm('cfg2')
    dev, host, _ = _engines(make_cfg2()[1], 64, diag, 2. * step, L)
    for engine in (dev, host): engine.set_adaptation(True, True)
    (_, _, idv), (_, _, ih) = run_batch(dev, 100, chunk=25), run_batch(host, 100, chunk=25)
    assert np.array_equal(idv[..., 1], ih[..., 1])
    eps_d, eps_h = dev.get_state()[4], host.get_state()[4]
    assert np.allclose(eps_d, eps_h, rtol=1e-10, atol=0.) and eps_h.std() > 0. and not np.allclose(eps_h, 2. * step)
    for a, b in zip(dev.get_moments(), host.get_moments()): assert np.allclose(a, b, rtol=1e-10, atol=1e-8)
    assert dev.get_moments()[0].min() > 0.


def test_mclmc_posterior_on_the_device():
    from desilike_amd.samplers import MCLMCSampler, EmceeSampler
    g, like = make_cfg2()
    names = like.varied_params.names()
    sampler = MCLMCSampler(like, chains=64, seed=2, adaptation={'niterations': 300})
    assert sampler.device_resident
    # cfg2's proposal scales are 17 to 90 times below the posterior's widths and the chains start from the narrow reference distributions: a warm-up of 300
    # iterations ends while they still spread, its preconditioner is too small by an order of magnitude and the autocorrelation time of the sampling run is about
    # 1000 steps (measured on the MI355X; with niterations 1000 it is 100 to 200).  The run is sized for that: 40000 steps (a few seconds), the first quarter dropped.
    chains = sampler.run(check_every=40000, max_iterations=40000, thin_by=20)
    # cfg2's posterior fills its uniform priors in qpar, qper, df and b1: steps that leave them are undone
    assert sampler.undone_steps.sum() > 0 and all(np.all(np.isfinite(chain['logposterior'])) for chain in chains)
    x = np.column_stack([np.concatenate([chain[name][500:] for chain in chains]) for name in names])
    ens = EmceeSampler(make_cfg2()[1], nwalkers=64, seed=3)
    chain = ens.run(niterations=1500)
    y = np.column_stack([chain[name][500:].ravel() for name in names])
    print('mean shift / sigma', (x.mean(axis=0) - y.mean(axis=0)) / y.std(axis=0), 'std ratio', x.std(axis=0) / y.std(axis=0), sampler.hyp, float(np.mean(sampler.acceptance_rate)))
    assert np.all(np.abs(x.mean(axis=0) - y.mean(axis=0)) < 0.3 * y.std(axis=0)), (x.mean(axis=0), y.mean(axis=0), y.std(axis=0))
    assert np.allclose(x.std(axis=0), y.std(axis=0), rtol=0.25)


def test_state_round_trip_and_errors():
    from desilike_amd._lib import DeviceMCLMC, LibraryError
    g, like = make_cfg2()
    ctx = like._get_context()
    P = ctx.n_params
    mclmc = DeviceMCLMC(ctx, 4, seed=3)
    start = np.array([[param.value for param in like.varied_params]] * 4) + 1e-3 * np.arange(4)[:, None]
    momenta = np.random.RandomState(0).standard_normal((4, P))
    momenta /= np.sqrt((momenta**2).sum(axis=1))[:, None]
    mclmc.set_preconditioner(np.ones(P) * 1e-2)
    mclmc.set_hyper(0.1, 2.)
    mclmc.set_state(start, momenta=momenta, counters=[5, 6, 7, 8])
    coords, u, logp, counters, eps = mclmc.get_state()
    assert np.array_equal(coords, start) and np.array_equal(u, momenta) and np.array_equal(counters, [5, 6, 7, 8]) and np.all(np.isfinite(logp)) and np.all(eps == 0.1)
    mclmc.set_state(start)      # momenta drawn from the counters: unit vectors, one per chain
    u = mclmc.get_state()[1]
    assert np.allclose((u**2).sum(axis=1), 1., rtol=0, atol=1e-14) and np.unique(u[:, 0]).size == 4
    bad = start.copy(); bad[1, 0] = np.nan
    with pytest.raises(LibraryError, match='finite'): mclmc.set_state(bad)
    with pytest.raises(LibraryError, match='unit'): mclmc.set_state(start, momenta=2. * momenta)
    with pytest.raises(LibraryError, match='nchains'): DeviceMCLMC(ctx, 0)
    with pytest.raises(ValueError, match='integrator'): DeviceMCLMC(ctx, 4, integrator='velocity_verlet')
    with pytest.raises(LibraryError, match='integrator'): DeviceMCLMC(ctx, 4, integrator=7)
    with pytest.raises(LibraryError, match='positive'): mclmc.set_preconditioner(-np.ones(P))
    with pytest.raises(LibraryError, match='step_size'): mclmc.set_hyper(0., 1.)
    fresh = DeviceMCLMC(ctx, 4)
    with pytest.raises(LibraryError, match='preconditioner'): fresh.run(1, 1, fresh.buffers(1))
    # the analytic mode outside the analytic gradient's scope (a context with analytically solved parameters)
    ctx5 = _cfg5()._get_context()
    analytic = DeviceMCLMC(ctx5, 2, gradient='analytic')
    analytic.set_preconditioner(np.ones(ctx5.n_params))
    with pytest.raises(LibraryError, match='analytic'):
        analytic.set_state(np.array([[param.value for param in _cfg5().varied_params]] * 2))
