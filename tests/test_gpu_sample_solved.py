"""GPU (-m gpu): posterior draws of analytically solved parameters (dl_sample_solved, desilike_amd.sample_solved).  The main check needs no oracle: loglike + logprior of
every draw must be the log-posterior of a context with NOTHING marginalised (the solved parameters varied, as Fisher builds it), evaluated at (theta, draw)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import solved_oracle as so

pytestmark = pytest.mark.gpu

SEED, NPOINTS, SIZE = 42, 64, 2


def _ref_theta(like, n, seed):
    rng = np.random.RandomState(seed)
    return np.column_stack([np.clip(param.ref.sample(size=n, random_state=rng), *param.prior.limits) for param in like.varied_params])


def _prior_precision(like):
    return np.array([param.prior.scale**(-2) if param.prior.dist == 'norm' else 0. for param in like.solved_params])


def _is_marg(like):
    return np.array([(param.derived.replace('.auto', like.solved_default) if param.derived.startswith('.auto') else param.derived).startswith('.marg') for param in like.solved_params])


def _full_context(like):
    """The context with nothing marginalised: the solved parameters appended to the theta columns (what Fisher builds, fisher.py:688-695)."""
    from desilike_amd._lib import Context
    return Context(like._spec({}, like._flatdata_list(), like._precision_input, vary_solved=True), device=like.device)


def _vary_solved_keys(cfg):
    """The same for a flat reference-side key set (tests/golden/boundary_*.npz): every linear input that feeds solved parameter s reads theta column P + s instead, the
    solved parameters get rows of the prior table (norm with the marginalisation's (loc, 1 / scale^2), or flat) and the marg.* keys go."""
    new = {key: np.array(value) for key, value in cfg.items() if not (key.startswith('marg.') or '.marg.' in key)}
    P, x0 = int(cfg['n_params'][0]), np.asarray(cfg['marg.x0'], dtype='f8')
    for key, index in cfg.items():
        if '.marg.' not in key: continue
        obs, name = key.split('.marg.')
        inputs = np.array(cfg['{}.in.{}'.format(obs, name)], dtype='f8').reshape(-1, 2)
        for row, s in zip(inputs, np.ravel(index)):
            if s >= 0: row[:] = (P + s, x0[s])
        new['{}.in.{}'.format(obs, name)] = inputs.reshape(np.shape(cfg['{}.in.{}'.format(obs, name)]))
    rows = [[1., -np.inf, np.inf, loc, prec**-0.5] if prec > 0. else [0., -np.inf, np.inf, 0., 1.] for loc, prec in np.reshape(cfg['marg.prior'], (-1, 2))]
    new['priors'] = np.concatenate([np.reshape(cfg['priors'], (-1, 5)), rows])
    new['n_params'] = np.array([P + len(rows)], dtype='i4')
    return new


def _eft_likelihood():
    """EFT-like Kaiser: counter terms '.marg' (one with a Gaussian prior, one flat), sn0 '.best': the generic Gram finalize with a determinant over part of the set."""
    from golden_utils import load_golden
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, EFTLikeKaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    g = load_golden('cfg2_shapefit_window_dense')
    theory = EFTLikeKaiserTracerPowerSpectrumMultipoles(template=ShapeFitPowerSpectrumTemplate(z=0.5))
    theory.init.params['ct0_2'].update(derived='.marg', prior=dict(dist='norm', loc=0., scale=30.))
    theory.init.params['ct2_2'].update(derived='.marg', prior=dict(dist='uniform'))
    theory.init.params['sn0_2'].update(derived='.best', prior=dict(dist='uniform'))
    for name in ['ct4_2', 'sn2_2', 'sn4_2']:
        theory.init.params[name].update(fixed=True, value=0.)
    obs = TracerPowerSpectrumMultipolesObservable(data=g['obs0']['flatdata'], kedges=np.linspace(0., 0.2, 41), ells=(0, 2, 4), wmatrix=g['obs0']['matrix_full'], kin=g['obs0']['kin'],
                                                  ellsin=(0, 2, 4), theory=theory, shotnoise=1e4)
    return ObservablesGaussianLikelihood(observables=[obs], covariance=g['covariance'])


def _cfg3_likelihood():
    """make_cfg3(marg=True) on data generated AT the default values x0 of the solved parameters (the theory at the parameters' values plus noise of the covariance).
    The marginalised value is assembled from the Gram matrix of [d~(x0); T~] as -G00 / 2 - quad / 2 - lin with G00 = chi2(x0): its rounding error is eps chi2(x0) in
    ABSOLUTE terms.  On the fixture's own data chi2(x0) is ~1e7 for every theta (the data hold counter and stochastic terms far from x0 = 0), and the marginalised value
    already differs from the context with nothing marginalised AT THE SOLUTION, before any draw, by up to 1.6e-8 -- above 1e-10 max(1, |logposterior|) at the points of
    a chain, where |logposterior| is 1 .. 100 (13 of 64 points drawn from the parameters' ref distributions, the worst at 1.0e-9; figures in DESIGN.md section 6j).
    With chi2(x0) of the order of the number of data that term is gone: measured 6.0e-11 at worst on the 64 points, of which the draw kernel's share is below 4e-11."""
    from test_host_api import make_cfg3
    g, like = make_cfg3(marg=True)
    theta0 = np.array([[param.value for param in like.varied_params]])
    flat = like._get_context().eval_batch_host(theta0, return_flattheory=True)[3][0]
    noise = np.random.RandomState(8).multivariate_normal(np.zeros(len(flat)), g['covariance'])
    return make_cfg3(marg=True, data=flat + noise)[1]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(marginalised context, context with nothing marginalised, theta [NPOINTS, P], likelihood or None) of a case, built once."""
    from desilike_amd._lib import Context
    like = None
    if name == 'cfg3':            # the tail of the emulated feature-Gram kernel, 5 solved parameters
        like = _cfg3_likelihood()
    elif name == 'cfg4_xi':       # 10 broadband terms '.marg': pass-through columns, NS = 10
        from test_host_api import make_cfg4
        like = make_cfg4('xi')[1]
        like.initialize()
        for param in like.observables[0].wmatrix.theory.init.params.select(basename='al*'):
            param.update(derived='.marg')
        like._invalidate()
        assert len(like.solved_params) == 10
    elif name == 'eft':
        like = _eft_likelihood()
        assert like.solved_params.names() == ['ct0_2', 'ct2_2', 'sn0_2'] and not like._solved_are_constant()
    elif name == 'constant':      # every solved derivative row is constant: the samplers take the posterior context, x^ and H_L come from the per-point path
        from golden_utils import load_golden
        from test_gpu_marg import make_marg_likelihood
        like = make_marg_likelihood(load_golden('marg_sn0_grid'), solved='.marg')
        assert like._solved_are_constant() and like._get_posterior_context()[0].n_solved == 0
    elif name == 'stacked':       # the stacked emulator layout, from the reference-side keys
        from test_gpu_boundary import load_fixture
        g, cfg = load_fixture('cfg3_stacked_bench')
        inside = g['theta'][:len(g['marg_c'])][np.isfinite(g['marg_c'])]      # the fixture's rows inside the priors (11): the points are convex combinations of two
        rng = np.random.RandomState(6)                                         # of them, inside the (box-shaped) support as well
        i, j, a = rng.randint(len(inside), size=NPOINTS), rng.randint(len(inside), size=NPOINTS), rng.uniform(size=(NPOINTS, 1))
        theta = a * inside[i] + (1. - a) * inside[j]
        return Context(cfg, device=0), Context(_vary_solved_keys(cfg), device=0), theta, None
    theta = _ref_theta(like, NPOINTS, seed=21)
    return like._get_context(), _full_context(like), theta, like


@pytest.mark.parametrize('name', ['cfg3', 'stacked', 'cfg4_xi', 'eft', 'constant'])
def test_full_posterior_identity(name):
    """For every draw, loglike + logprior of dl_sample_solved = dl_eval_logposterior of the context with nothing marginalised at (theta, x), to 1e-10 max(1, |.|)."""
    ctx, full, theta, like = _case(name)
    ns = ctx.n_solved
    assert ns >= 1 and full.n_solved == 0 and full.n_params == ctx.n_params + ns
    x, loglike, logprior, status = ctx.sample_solved(theta, index0=0, size=SIZE, seed=SEED)
    assert x.shape == (NPOINTS, SIZE, ns) and loglike.shape == logprior.shape == (NPOINTS, SIZE)
    assert (status == 0).all()
    ref, status_ref = full.eval_logposterior_host(np.concatenate([np.repeat(theta, SIZE, axis=0), x.reshape(-1, ns)], axis=1))
    assert (status_ref == 0).all()
    got = (loglike + logprior).ravel()
    err = np.abs(got - ref) / np.maximum(1., np.abs(ref))
    print('{}: ns = {:d}, max |dl_sample_solved - full posterior| / max(1, |.|) = {:.3e}'.format(name, ns, err.max()))
    assert (err <= 1e-10).all(), err.max()
    # the draws moved: the identity is not the one at the solution
    xhat = ctx.eval_batch_derived_host(theta)[3]
    assert (np.abs(x - xhat[:, None, :]) > 0.).all()
    at_solution = full.eval_logposterior_host(np.concatenate([theta, xhat], axis=1))[0]      # full(theta, x) = full(theta, x^) - |z|^2 / 2: below the maximum
    assert (at_solution[:, None] - (loglike + logprior) >= -1e-9 * np.maximum(1., np.abs(at_solution[:, None]))).all()


def test_draws_vs_oracle():
    """cfg3: x^ and H_L from dl_eval_batch_derived, z from the Python mirror of the draw addressing; |C^T (x - x^) - z| <= 100 cond(A) eps per component with NumPy's
    Cholesky factor (the condition -- the bound below 1e-9 -- first), and the corrections against the restatement of chain.py:251-262."""
    ctx, full, _, like = _case('cfg3')
    ns, index0 = ctx.n_solved, 1000
    prec, marg = _prior_precision(like), _is_marg(like)
    # the inputs: the first NPOINTS of 160 points drawn from the ref distributions whose A meets the condition (cond(A) depends on theta: 2e4 .. 9e4 here)
    pool = _ref_theta(like, 160, seed=23)
    keep = np.flatnonzero([so.draw_bound(h, prec)[1] < 1e-9 for h in ctx.eval_batch_derived_host(pool)[4]])[:NPOINTS]
    assert len(keep) == NPOINTS, 'the inputs are at fault: {:d} of 160 points meet the condition'.format(len(keep))
    theta = pool[keep]
    x, loglike, logprior, status = ctx.sample_solved(theta, index0=index0, size=SIZE, seed=SEED)
    assert (status == 0).all()
    ll0, lp0, st0, xhat, hessian = ctx.eval_batch_derived_host(theta)
    z = so.gauss(SEED, index0 + np.arange(NPOINTS), np.arange(SIZE), ns)
    worst = 0.
    for b in range(NPOINTS):
        C, bound = so.draw_bound(hessian[b], prec)
        assert bound < 1e-9, 'the inputs are at fault: cond(A) = {:.3g}'.format(bound / 100. / so.EPS)
        resid = np.abs((x[b] - xhat[b]).dot(C) - z[b]).max()
        worst = max(worst, resid / bound)
        assert resid <= bound, (b, resid, bound)
        xo, dll, dlp = so.sample_solved(xhat[b], hessian[b], prec, marg, z[b])
        assert np.allclose(loglike[b], ll0[b] + dll, rtol=1e-10, atol=0.) and np.allclose(logprior[b], lp0[b] + dlp, rtol=1e-10, atol=1e-12)
    print('max residual / bound = {:.3e}'.format(worst))


def test_chunk_and_index_invariance():
    """B = 300 in one call = two calls with index0 = 0 and index0 = 137, bit for bit; B = 65: one lane beyond a wavefront; two calls give identical bits; draw d of
    size 2 is draw d of size 1."""
    ctx, full, theta, like = _case('cfg3')
    big = _ref_theta(like, 300, seed=22)
    whole = ctx.sample_solved(big, index0=0, size=SIZE, seed=SEED)
    first, second = ctx.sample_solved(big[:137], index0=0, size=SIZE, seed=SEED), ctx.sample_solved(big[137:], index0=137, size=SIZE, seed=SEED)
    for w, a, b in zip(whole, first, second):
        assert np.array_equal(w, np.concatenate([a, b]))
    again = ctx.sample_solved(big, index0=0, size=SIZE, seed=SEED)
    for w, a in zip(whole, again):
        assert np.array_equal(w, a)
    part = ctx.sample_solved(big[:65], index0=0, size=SIZE, seed=SEED)
    for w, p in zip(whole, part):
        assert np.array_equal(w[:65], p)
    assert np.isfinite(part[0]).all() and (part[3] == 0).all()
    one = ctx.sample_solved(big[:65], index0=0, size=1, seed=SEED)
    for w, p in zip(part[:3], one[:3]):
        assert np.array_equal(w[:, :1], p)
    other = ctx.sample_solved(big[:65], index0=0, size=SIZE, seed=SEED + 1)
    assert not np.isclose(other[0], part[0]).any()
    shifted = ctx.sample_solved(big[:65], index0=1, size=SIZE, seed=SEED)
    assert not np.isclose(shifted[0], part[0]).any()


def test_bad_rows():
    """One row outside its prior and one with a NaN parameter among good rows: NaN draws and values, non-zero status; the rows beside them are bit-identical to a call
    in which those rows are good."""
    ctx, full, theta, like = _case('cfg3')
    good = ctx.sample_solved(theta, index0=0, size=SIZE, seed=SEED)
    bad = theta.copy()
    limits = like.varied_params[0].prior.limits
    assert np.isfinite(limits[1])
    bad[3, 0] = limits[1] + 1.
    bad[40, 1] = np.nan
    x, loglike, logprior, status = ctx.sample_solved(bad, index0=0, size=SIZE, seed=SEED)
    assert status[3] == 1 and status[40] == 3 and np.count_nonzero(status) == 2
    keep = np.ones(NPOINTS, dtype='?')
    keep[[3, 40]] = False
    for row in (3, 40):
        assert np.isnan(x[row]).all() and np.isnan(loglike[row]).all() and np.isnan(logprior[row]).all()
    for new, old in zip((x, loglike, logprior), good):
        assert np.array_equal(new[keep], old[keep])
    import desilike_amd
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        new = desilike_amd.sample_solved(like, {param.name: bad[:, i] for i, param in enumerate(like.varied_params)}, size=SIZE, seed=SEED)
    assert any('2 chain points' in str(w.message) for w in caught)
    name = like.solved_params.names()[0]
    assert np.isnan(new[name][6:8]).all() and np.array_equal(new[name].reshape(NPOINTS, SIZE)[keep], x[keep][..., 0])


def test_context_without_solved_parameters():
    """The entry returns 2 with nothing launched; the Python surface raises ValueError."""
    import torch
    import desilike_amd
    from test_host_api import make_cfg3
    like = make_cfg3(marg=False)[1]
    ctx = like._get_context()
    assert ctx.n_solved == 0
    theta = torch.as_tensor(_ref_theta(like, 8, seed=1), dtype=torch.float64, device='cuda:0').contiguous()
    out = torch.full((8, 1, 1), 7., dtype=torch.float64, device='cuda:0')
    rc = ctx._lib.dl_sample_solved(ctx._handle, ctypes.c_void_p(theta.data_ptr()), 8, 0, 1, 42, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.c_void_p(out.data_ptr()), None, None)
    torch.cuda.synchronize()
    assert rc == 2 and (out.cpu().numpy() == 7.).all()
    with pytest.raises(ValueError):
        ctx.sample_solved(theta)
    with pytest.raises(ValueError):
        desilike_amd.sample_solved(like, {param.name: np.full(4, param.value) for param in like.varied_params})
    with pytest.raises(ValueError):
        _case('cfg3')[0].sample_solved(_case('cfg3')[2], size=0)


def _spot_check(like, full, new, rows):
    names = like.varied_params.names() + like.solved_params.names()
    point = np.column_stack([np.ravel(new[name])[rows] for name in names])
    ref = full.eval_logposterior_host(point)[0]
    got = np.ravel(new['logposterior'])[rows]
    print('spot check: max |sample_solved - full posterior| / max(1, |.|) = {:.3e} on {:d} rows, |logposterior| {:.3g} .. {:.3g}'.format(
        (np.abs(got - ref) / np.maximum(1., np.abs(ref))).max(), len(rows), np.abs(ref).min(), np.abs(ref).max()))
    assert (np.abs(got - ref) <= 1e-10 * np.maximum(1., np.abs(ref))).all(), np.abs(got - ref).max()
    assert np.array_equal(np.ravel(new['loglikelihood'] + new['logprior'])[rows], got)


def test_end_to_end_samplers():
    """A short EmceeSampler and a short NestedSampler on the marginalised cfg3 likelihood, then sample_solved(size=2): shapes, weights, and the identity on 32 rows."""
    import desilike_amd
    from desilike_amd.samplers import EmceeSampler
    from desilike_amd.nested import NestedSampler
    ctx, full, theta, like = _case('cfg3')
    solved = like.solved_params.names()
    sampler = EmceeSampler(like, nwalkers=64, seed=5)
    chain = sampler.run(niterations=6)
    new = desilike_amd.sample_solved(like, sampler.chain, size=2, seed=SEED)
    shape = np.shape(sampler.chain['logposterior'])
    assert shape == (6, 64)
    for name in like.varied_params.names() + solved + ['loglikelihood', 'logprior', 'logposterior']:
        assert new[name].shape == (6, 128), name
    assert np.array_equal(new[like.varied_params.names()[0]], np.repeat(sampler.chain[like.varied_params.names()[0]], 2, axis=1))
    finite = np.flatnonzero(np.isfinite(np.ravel(new['logposterior'])))
    _spot_check(like, full, new, finite[np.linspace(0, len(finite) - 1, 32).astype(int)])
    # the sampler itself, and the method of Samples, give the same
    both = desilike_amd.sample_solved(like, sampler, size=2, seed=SEED)
    assert isinstance(both, list) and len(both) == 1 and all(np.array_equal(both[0][name], new[name]) for name in new)
    nested = NestedSampler(like, nlive=64, ndelete=32, n_steps=8, dlogz=0.5, seed=3)
    nested.run()
    dead = nested.chains[0]
    new = desilike_amd.Samples(dead).sample_solved(like, size=2, seed=SEED)
    n = len(dead['logposterior'])
    for name in solved + ['loglikelihood', 'logposterior', 'logweight', 'aweight']:
        assert new[name].shape == (2 * n,), name
    assert np.array_equal(new['aweight'], np.repeat(dead['aweight'], 2)) and np.array_equal(new['logweight'], np.repeat(dead['logweight'], 2))
    # the 32 rows that carry the most posterior weight: the rows a posterior estimate is made of (the first dead points of a run come from the prior, with weights
    # of e^-1000 and below, far from the expansion point of the emulator, where the marginalised value and the full one agree less well: _cfg3_likelihood)
    _spot_check(like, full, new, np.argsort(new['aweight'], kind='stable')[-32:])
