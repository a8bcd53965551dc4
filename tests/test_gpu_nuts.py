"""GPU: the device-resident No-U-Turn sampler (dl_nuts_*, desilike_amd/nuts.py _DeviceNUTS) against the NumPy statement of the same step (_HostNUTS) fed by the same
device gradient, its asynchronous chains, its posterior, its state and errors."""
import numpy as np
import pytest

from test_host_api import make_cfg2, make_cfg5

pytestmark = pytest.mark.gpu


def _engines(like, nchains, minv, step, gradient='auto', max_num_doublings=10, seed=5):
    """(_DeviceNUTS, _HostNUTS) on the same chains; the host's gradient is the context's own on the same rows (analytic, or central differences through
    dl_eval_logposterior on the stencil the device builds)."""
    import torch
    from desilike_amd.nuts import NUTSSampler, _DeviceNUTS, _HostNUTS
    sampler = NUTSSampler(like, chains=nchains, adaptation=False, gradient=gradient, seed=seed)
    ctx, offset = like._get_posterior_context()
    delta, limits = sampler._fd_tables()
    ids = np.arange(nchains)
    dev = _DeviceNUTS(ctx, offset, ids, max_num_doublings, 1000., seed, gradient, delta, limits)

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

    host = _HostNUTS(f, nchains, len(like.varied_params), chain_ids=ids, max_num_doublings=max_num_doublings, seed=seed, offset=offset)
    start = sampler._get_start(nchains)[0]
    for engine in (dev, host):
        engine.set_mass(minv, step)
        engine.set_state(start)
    return dev, host, sampler


def _warm(like_builder, nchains=64, niterations=100):
    """Hyper-parameters from a short warm-up on the device: (diagonal, dense inverse mass matrix, step size)."""
    from desilike_amd.samplers import NUTSSampler
    s = NUTSSampler(like_builder(), chains=nchains, seed=11, adaptation={'niterations': niterations, 'is_mass_matrix_diagonal': False})
    s.run(check_every=50, max_iterations=50)
    x = np.concatenate([np.column_stack([c[n] for n in s.varied_params.names()]) for c in s.chains])
    return np.diag(s.inverse_mass_matrix).copy(), np.asarray(s.inverse_mass_matrix), s.step_size, x.std(axis=0)


def _compare(dev, host, niterations, std, chunk=32):
    from desilike_amd.nuts import run_batch
    cd, ld, idv = run_batch(dev, niterations, chunk=chunk)
    ch, lh, ih = run_batch(host, niterations, chunk=chunk)
    assert np.array_equal(idv[..., :3], ih[..., :3]), 'tree depths / leapfrog counts / divergence flags differ'
    assert np.all(np.abs(cd - ch) <= 1e-9 * std), float(np.max(np.abs(cd - ch) / std))
    assert np.allclose(ld, lh, rtol=1e-10, atol=1e-8)
    return idv


@pytest.mark.parametrize('dense', [False, True])
def test_device_equals_the_host_driver(dense):
    diag, full, step, std = _warm(lambda: make_cfg2()[1])
    g, like = make_cfg2()
    dev, host, _ = _engines(like, 64, full if dense else diag, step)
    info = _compare(dev, host, 150, std)
    assert info[..., 0].max() >= 2 and info[..., 1].sum() > 64 * 150


def test_finite_difference_route_equals_the_host_driver():
    """Central differences (gradient='finite') on a marginalised likelihood (the constant of the marginalisation travels as the offset): the device differentiates
    through dl_eval_logposterior on its stencil."""
    def build():
        g, like = make_cfg5()
        like.all_params = {'*.sn0': {'derived': '.marg'}}
        return like

    diag, _, step, std = _warm(build, nchains=32, niterations=60)
    dev, host, _ = _engines(build(), 32, diag, step, gradient='finite')
    _compare(dev, host, 40, std)
    assert dev.nuts.info('finite') == 1


def test_chains_are_asynchronous():
    from desilike_amd.nuts import run_batch
    diag, _, step, _ = _warm(lambda: make_cfg2()[1])
    for depth in (2, 10):
        dev, _, _ = _engines(make_cfg2()[1], 64, diag, step, max_num_doublings=depth)
        buffers = dev.buffers(60)
        while True:
            dev.run(16, 60, buffers)
            counts = dev.counts(buffers)
            if np.all(counts >= 60): break
        assert np.all(counts == 60)
        info = dev.records(buffers)[2]
        assert info[..., 0].max() <= depth
        per_chain = info[..., 1].sum(axis=1)
        # shallow trees do not wait for deep ones: the steps enqueued are the slowest chain's leapfrog total, to one chunk
        assert per_chain.max() <= dev.steps <= per_chain.max() + 16, (dev.steps, per_chain.max(), per_chain.min())
    # the chunking does not change the chains
    a, _, _ = _engines(make_cfg2()[1], 64, diag, step)
    b, _, _ = _engines(make_cfg2()[1], 64, diag, step)
    ra, rb = run_batch(a, 40, chunk=7), run_batch(b, 40, chunk=64)
    for x, y in zip(ra, rb): assert np.array_equal(x, y)


def test_nuts_posterior_on_the_device():
    from desilike_amd.samplers import NUTSSampler, EmceeSampler
    g, like = make_cfg2()
    names = like.varied_params.names()
    sampler = NUTSSampler(like, chains=64, seed=2, adaptation={'niterations': 200}, gradient='analytic')
    assert sampler.device_resident
    chains = sampler.run(check_every=150, max_iterations=300)
    # cfg2's posterior fills its uniform priors in qpar, qper, df and b1: most trajectories end at a prior bound (divergent: a leaf outside the support, as Stan
    # and blackjax count it); energy errors are rare (1 transition in 19200 on the MI355X)
    assert 0.5 < sampler.acceptance_rate.mean() <= 1. and sampler.energy_divergences.sum() < 1e-3 * 64 * 300
    x = np.column_stack([np.concatenate([chain[name][100:] for chain in chains]) for name in names])
    ens = EmceeSampler(make_cfg2()[1], nwalkers=64, seed=3)
    chain = ens.run(niterations=1500)
    y = np.column_stack([chain[name][500:].ravel() for name in names])
    assert np.all(np.abs(x.mean(axis=0) - y.mean(axis=0)) < 0.25 * y.std(axis=0)), (x.mean(axis=0), y.mean(axis=0), y.std(axis=0))
    assert np.allclose(x.std(axis=0), y.std(axis=0), rtol=0.25)
    assert sampler.mean_tree_depth.mean() >= 1.


def test_state_round_trip_and_errors():
    from desilike_amd._lib import DeviceNUTS, LibraryError
    g, like = make_cfg2()
    ctx = like._get_context()
    P = ctx.n_params
    nuts = DeviceNUTS(ctx, 4, seed=3)
    start = np.array([[param.value for param in like.varied_params]] * 4) + 1e-3 * np.arange(4)[:, None]
    nuts.set_mass(np.ones(P) * 1e-2, 0.1)
    nuts.set_state(start, iterations=[5, 6, 7, 8])
    coords, logp, iterations, logeps = nuts.get_state()
    assert np.array_equal(coords, start) and np.array_equal(iterations, [5, 6, 7, 8]) and np.all(np.isfinite(logp)) and np.allclose(logeps, np.log(0.1))
    bad = start.copy(); bad[1, 0] = np.nan
    with pytest.raises(LibraryError, match='finite'): nuts.set_state(bad)
    with pytest.raises(LibraryError, match='nchains'): DeviceNUTS(ctx, 0)
    with pytest.raises(LibraryError, match='max_num_doublings'): DeviceNUTS(ctx, 4, max_num_doublings=0)
    with pytest.raises(LibraryError, match='positive definite'): nuts.set_mass(-np.eye(P), 0.1)
    # the analytic mode outside the analytic gradient's scope (a context with analytically solved parameters)
    g5, like5 = make_cfg5()
    like5.all_params = {'*.sn0': {'derived': '.marg'}}
    ctx5 = like5._get_context()
    analytic = DeviceNUTS(ctx5, 2, gradient='analytic')
    analytic.set_mass(np.ones(ctx5.n_params), 0.1)
    with pytest.raises(LibraryError, match='analytic'):
        analytic.set_state(np.array([[param.value for param in like5.varied_params]] * 2))
