"""GPU (-m gpu): dl_eval_fisher_analytic on emulated full-shape likelihoods (csrc/dl_emu_jac.h: tangent kernel -> U GEMM -> row kernel -> MFMA Gram product), through
``Context.eval_fisher_analytic``, ``Fisher(method='analytic')`` and ``GaussNewtonProfiler(derivatives='analytic')``, against the exact Jacobian of the torch oracle
(tests/emu_jac_oracle.py).  Bounds: Hessian and gradient 1e-8 of the largest entry (tests/test_gpu_fisher_analytic.py); offset 1e-9 max(1, |ref|)
(tests/test_gpu_emulated_grad.py; ``offset_ref`` is the log-likelihood -1/2 D P D, the device's offset is -D P D as everywhere in this package, so half of it is compared);
Fisher gradient against the merged analytic gradient 1e-10 of the largest component.  Every test first asserts that the analytic entry answers."""
import functools
import warnings

import numpy as np
import pytest

from bench_configs import make_cfg3_full, make_cfg3_stacked
from emulator_utils import CFG3_PARAMS, EMU_PARAMS
from emu_jac_oracle import EmulatedJacobianOracle
from test_gpu_emulator import make_mlp_likelihood

pytestmark = pytest.mark.gpu


def _fisher(like, method='analytic'):
    from desilike_amd.fisher import Fisher
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # (solved parameters are varied: test_solved_parameters_varied checks the warning itself)
        return Fisher(like, method=method)


def _centres(fisher, n, seed):
    """As ``_theta`` of tests/test_gpu_emulated_grad.py, over the columns of the Fisher context (varied, then solved)."""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(np.column_stack([np.clip(param.ref.sample(size=n, random_state=rng), *param.prior.limits) for param in fisher.varied_params]))


def _device(fisher, centres, **kwargs):
    import torch
    ctx = fisher._get_context()
    out = ctx.eval_fisher_analytic(torch.as_tensor(centres, device=torch.device('cuda', ctx.device)).contiguous(), **kwargs)
    assert out is not None
    return out


def _numpy(out):
    return [a.cpu().numpy() for a in out]


def _check_rows(oracle, centres, hessian, gradient, offset, rows, cache=None, tag=''):
    for i in rows:
        key = centres[i].tobytes()
        if cache is None or key not in cache:
            ref = oracle.fisher(centres[i])
            if cache is not None: cache[key] = ref
        else: ref = cache[key]
        roffset, rgradient, rhessian, J = ref
        herr, gerr = np.abs(hessian[i] - rhessian).max() / np.abs(rhessian).max(), np.abs(gradient[i] - rgradient).max() / np.abs(rgradient).max()
        oerr = abs(0.5 * offset[i] - roffset) / max(1., abs(roffset))
        print('{} row {:d}: hessian {:.2e}, gradient {:.2e} of the largest entry, offset {:.2e}'.format(tag, i, herr, gerr, oerr))
        assert herr <= 1e-8 and gerr <= 1e-8, (i, herr, gerr)
        assert oerr <= 1e-9, (i, offset[i], roffset)
        assert np.array_equal(hessian[i], hessian[i].T)


ARCHITECTURES = [((8,), 'silu'), ((5, 7, 3), 'silu'), ((24, 40), 'tanh'), ((100,), 'relu'), ((64, 32), 'silu'), ((128, 128, 128, 128, 128), 'silu'),
                 ((16, 16, 16, 16, 16, 16, 16), 'tanh')]


@pytest.mark.parametrize('marg', [True, False])
@pytest.mark.parametrize('hidden,activation', ARCHITECTURES)
def test_mlp_architectures(hidden, activation, marg):
    import torch
    g, like, pt, theory, solved = make_mlp_likelihood(marg=marg, seed=5, hidden=hidden, activation=activation)
    fisher = _fisher(like)
    centres = _centres(fisher, 257, 6)
    oracle = EmulatedJacobianOracle(like, pt, theory, EMU_PARAMS, 'lpt', fisher.varied_params.names())
    cache, outs = {}, {}
    for B, rows in [(1, (0,)), (17, (0, 16)), (257, (0, 15, 16, 255, 256))]:
        first = [a.clone() for a in _device(fisher, centres[:B])]
        second = _device(fisher, centres[:B])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, second))           # two calls: the same bits
        hessian, gradient, offset = _numpy(first)
        assert np.isfinite(hessian).all() and np.isfinite(gradient).all() and np.isfinite(offset).all()
        assert all(np.array_equal(h, h.T) for h in hessian)
        _check_rows(oracle, centres, hessian, gradient, offset, rows, cache=cache, tag='{} {} marg={} B={:d}'.format(hidden, activation, marg, B))
        outs[B] = (offset, gradient, hessian)
    # through Fisher: the same numbers as the same batch through the context
    assert all(np.array_equal(a, b) for a, b in zip(fisher.evaluate(centres[:17]), outs[17]))


@pytest.mark.parametrize('hidden,activation', [((24, 40), 'tanh'), ((64, 32), 'silu'), ((100,), 'relu')])
def test_fisher_gradient_is_the_merged_analytic_gradient(hidden, activation):
    """No solved parameter: the Fisher gradient of the likelihood term is dl_eval_logposterior_grad (csrc/dl_emu_grad.h, reverse mode) minus the prior gradient."""
    from desilike_amd.fisher import logposterior_value_and_grad
    g, like, pt, theory, solved = make_mlp_likelihood(marg=False, seed=5, hidden=hidden, activation=activation)
    fisher = _fisher(like)
    centres = _centres(fisher, 40, 11)
    hessian, gradient, offset = _numpy(_device(fisher, centres))
    value, grad = logposterior_value_and_grad(like, centres, method='analytic')
    inside = np.isfinite(value)
    assert inside.sum() >= 20
    prior_gradient = np.zeros_like(centres)
    for ip, param in enumerate(like.varied_params):
        if param.prior.dist == 'norm': prior_gradient[:, ip] = -(centres[:, ip] - param.prior.loc) / param.prior.scale**2
        else: assert param.prior.dist == 'uniform'
    err = np.abs(gradient - (grad - prior_gradient))[inside].max(axis=1) / np.abs(gradient[inside]).max(axis=1)
    print('{} {}: Fisher gradient vs merged analytic gradient: max {:.2e}'.format(hidden, activation, err.max()))
    assert (err <= 1e-10).all()


def test_solved_parameters_varied():
    """'.marg' / '.best' mixes (the kinds of test_best_marg_mix_gradient): Fisher warns and carries the solved columns; the block of the sn* columns, whose derivative rows
    do not depend on the centre (their tables are constants), is the oracle's constant -J_s P J_t at every centre."""
    from desilike_amd.fisher import Fisher
    kinds = {'alpha0p': '.best', 'alpha2p': '.marg', 'sn0p': '.marg', 'sn2p': '.best'}
    g, like, pt, theory, solved = make_mlp_likelihood(derived=kinds, seed=2)
    with pytest.warns(UserWarning, match='solved parameters'):
        fisher = Fisher(like, method='analytic')
    names = fisher.varied_params.names()
    assert sorted(names[-len(kinds):]) == sorted(kinds) and names[:-len(kinds)] == like.varied_params.names() and fisher._get_context().n_solved == 0
    centres = _centres(fisher, 100, 8)
    hessian, gradient, offset = _numpy(_device(fisher, centres))
    oracle = EmulatedJacobianOracle(like, pt, theory, EMU_PARAMS, 'lpt', names)
    cache = {}
    _check_rows(oracle, centres, hessian, gradient, offset, (0, 17, 99), cache=cache, tag='best/marg mix')
    isn = [names.index('sn0p'), names.index('sn2p')]
    J = [cache[centres[i].tobytes()][3][:, isn] for i in (0, 17, 99)]
    assert all(np.abs(Ji - J[0]).max() <= 1e-12 * np.abs(J[0]).max() for Ji in J[1:])          # the oracle's rows of sn0p, sn2p are constants
    block = -J[0].T @ np.asarray(like.precision) @ J[0]
    assert (np.abs(hessian[:, isn][:, :, isn] - block).max(axis=(1, 2)) <= 1e-8 * np.abs(block).max()).all()
    # every alpha* / sn* column against the oracle's derivative row, through the Hessian column it makes with all the others
    for name in kinds:
        i = names.index(name)
        for ic in (0, 17, 99):
            Jc = cache[centres[ic].tobytes()][3]
            ref = -Jc.T @ np.asarray(like.precision) @ Jc[:, i]
            assert np.abs(hessian[ic][:, i] - ref).max() <= 1e-8 * np.abs(hessian[ic]).max(), (name, ic)


def test_parameter_reaching_no_theory_leaves_exact_zeros():
    """sn4p varied while the emulated tables of its monomial are zero (test_parameter_reaching_no_theory_gets_prior_gradient_only): Hessian row and column and gradient
    entry exactly zero."""
    g, like, pt, theory, solved = make_mlp_likelihood(marg=True, seed=5)
    table = pt.engines['pktable']
    yl = np.array(table.ylimits, dtype='f8').reshape(3, -1, 19, 2)
    yl[:, :, 18, :] = 0.
    table.ylimits = yl.reshape(-1, 2)
    theory.init.params['sn4p'].update(fixed=False, prior={'dist': 'norm', 'loc': 0.1, 'scale': 2.}, ref={'limits': [-0.5, 0.5]})
    fisher = _fisher(like)
    names = fisher.varied_params.names()
    i = names.index('sn4p')
    centres = _centres(fisher, 40, 9)
    hessian, gradient, offset = _numpy(_device(fisher, centres))
    assert np.isfinite(hessian).all() and np.isfinite(offset).all()
    assert (hessian[:, i, :] == 0.).all() and (hessian[:, :, i] == 0.).all() and (gradient[:, i] == 0.).all()
    other = [j for j in range(len(names)) if j != i]
    assert (np.abs(hessian[:, other][:, :, other]).max(axis=(1, 2)) > 0.).all()
    oracle = EmulatedJacobianOracle(like, pt, theory, EMU_PARAMS, 'lpt', names)
    _check_rows(oracle, centres, hessian, gradient, offset, (0, 39), tag='sn4p without tables')


@pytest.mark.parametrize('marg', [False, True])
def test_taylor_engines(marg):
    """The reference-pinned fixture of tests/test_host_api.py: table, sigma8 and fsigma8 engines exact second-order polynomials (REPT tracer), so the oracle's Jacobian is
    closed form."""
    from test_host_api import make_cfg3
    g, like = make_cfg3(marg=marg)
    like.initialize()
    theory = like.observables[0].wmatrix.theory
    fisher = _fisher(like)
    centres = _centres(fisher, 17, 12)
    hessian, gradient, offset = _numpy(_device(fisher, centres))
    oracle = EmulatedJacobianOracle(like, theory.pt, theory, EMU_PARAMS, 'rept', fisher.varied_params.names())
    _check_rows(oracle, centres, hessian, gradient, offset, (0, 15, 16), tag='taylor marg={}'.format(marg))


def test_cfg3_full_1024():
    g, like, pt, theory, solved = make_cfg3_full(marg=True)
    fisher = _fisher(like)
    centres = _centres(fisher, 1024, 3)
    hessian, gradient, offset = _numpy(_device(fisher, centres))
    assert np.isfinite(hessian).all()
    oracle = EmulatedJacobianOracle(like, pt, theory, CFG3_PARAMS, 'rept', fisher.varied_params.names())
    _check_rows(oracle, centres, hessian, gradient, offset, (0, 15, 16, 255, 256, 1023), tag='cfg3 full')


def test_plumbing():
    """5000 centres of a small network: the pass split is crossed (the pass count asserted from the rule); slices from either side of a split; each output alone; a
    NaN centre."""
    import torch
    g, like, pt, theory, solved = make_mlp_likelihood(marg=False, seed=5, hidden=(8,))
    fisher = _fisher(like)
    ctx = fisher._get_context()
    device = torch.device('cuda', ctx.device)
    P = len(fisher.varied_params)
    out = ctx.eval_fisher_analytic(torch.empty((0, P), dtype=torch.float64, device=device))
    assert out is not None and out[0].shape == (0, P, P) and out[1].shape == (0, P) and out[2].shape == (0,)
    # the rule (dl_api.hip): pass x max((1 + n_xv) x 19 x N_pad, (1 + P) x N_pad) <= 16 Mi doubles, at most 2048, whole 64-row tiles
    n_xv, N_pad = len(EMU_PARAMS), ctx.info('N_pad')
    per_pass = max(64, min(2048, (16 << 20) // max((1 + n_xv) * 19 * N_pad, (1 + P) * N_pad)) // 64 * 64)
    assert ctx.info('fisher_analytic_pass') == per_pass == 1664
    B = 5000
    assert -(-B // per_pass) == 4
    big = _centres(fisher, B, 4)
    t = torch.as_tensor(big, device=device).contiguous()
    first = [a.clone() for a in ctx.eval_fisher_analytic(t)]
    second = ctx.eval_fisher_analytic(t)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(bool(torch.isfinite(a).all()) for a in first)

    def close(a, b):
        return bool((a - b).abs().max() <= 1e-11 * b.abs().max())

    for n in (1, 17):
        for start in (0, per_pass - n, per_pass, B - n):          # (either side of the first split, and the end of the last, shorter pass)
            part = ctx.eval_fisher_analytic(t[start:start + n].contiguous())
            assert all(a.shape[0] == n and close(a, b[start:start + n]) for a, b in zip(part, first)), (n, start)
    full = [a.clone() for a in ctx.eval_fisher_analytic(t[:17].contiguous())]
    only_h = ctx.eval_fisher_analytic(t[:17].contiguous(), gradient=False, offset=False)
    only_g = ctx.eval_fisher_analytic(t[:17].contiguous(), hessian=False, offset=False)
    only_o = ctx.eval_fisher_analytic(t[:17].contiguous(), hessian=False, gradient=False)
    none = ctx.eval_fisher_analytic(t[:17].contiguous(), hessian=False, gradient=False, offset=False)
    torch.cuda.synchronize()
    assert only_h[1] is None and only_h[2] is None and torch.equal(only_h[0], full[0]) and only_g[0] is None and torch.equal(only_g[1], full[1])
    assert only_o[0] is None and torch.equal(only_o[2], full[2]) and none == (None, None, None)
    # one NaN centre: NaN outputs for it, the others as before
    bad = big[:3].copy(); bad[1, fisher.varied_params.names().index('qper')] = np.nan
    out = _numpy(ctx.eval_fisher_analytic(torch.as_tensor(bad, device=device).contiguous()))
    assert np.isnan(out[2][1]) and np.isnan(out[1][1]).all() and np.isnan(out[0][1]).any()
    assert all(np.isfinite(a[[0, 2]]).all() and np.allclose(a[[0, 2]], b[[0, 2]].cpu().numpy(), rtol=0., atol=1e-11 * float(b[[0, 2]].abs().max())) for a, b in zip(out, first))


def _two_emulated_observables():
    from desilike_amd.theories.galaxy_clustering import LPTVelocileptorsTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    g, like, pt, theory, solved = make_mlp_likelihood(marg=False, seed=5, hidden=(8,))
    observables = []
    for tracer in ('ELG', 'LRG'):
        theory = LPTVelocileptorsTracerPowerSpectrumMultipoles(pt=pt, tracer=tracer)
        theory.init.params['sn4p'].update(fixed=True, value=0.3)
        observables.append(TracerPowerSpectrumMultipolesObservable(data=g['obs0']['flatdata'], kedges=np.linspace(0.02, 0.2, 37), ells=(0, 2, 4), wmatrix={'resolution': 2}, theory=theory,
                                                                   shotnoise=8e3))
    cov = np.asarray(g['covariance'], dtype='f8')
    n = cov.shape[0]
    covariance = np.zeros((2 * n, 2 * n)); covariance[:n, :n] = cov; covariance[n:, n:] = cov
    return ObservablesGaussianLikelihood(observables=observables, covariance=covariance)


def _emulated_with_transform():
    from desilike_amd.theories.galaxy_clustering import LPTVelocileptorsTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    g, like, pt, theory, solved = make_mlp_likelihood(marg=False, seed=5, hidden=(8,))
    theory = LPTVelocileptorsTracerPowerSpectrumMultipoles(pt=pt, tracer='ELG')
    theory.init.params['sn4p'].update(fixed=True, value=0.3)
    obs = TracerPowerSpectrumMultipolesObservable(data=g['obs0']['flatdata'], kedges=np.linspace(0.02, 0.2, 37), ells=(0, 2, 4), wmatrix={'resolution': 2}, theory=theory, shotnoise=8e3,
                                                  transform='cubic')
    return ObservablesGaussianLikelihood(observables=[obs], covariance=g['covariance'])


@functools.lru_cache(maxsize=None)
def _out_of_scope(name):
    if name == 'stacked': return make_cfg3_stacked(marg=True, hidden=(32, 32), nk=30, seed=4)[0]
    if name == 'two_observables': return _two_emulated_observables()
    return _emulated_with_transform()


@pytest.mark.parametrize('name', ['stacked', 'two_observables', 'transform'])
def test_scope(name):
    import torch
    like = _out_of_scope(name)
    like.initialize()
    fisher = _fisher(like)
    ctx = fisher._get_context()
    centres = _centres(fisher, 2, 1)
    assert ctx.eval_fisher_analytic(torch.as_tensor(centres, device=torch.device('cuda', ctx.device)).contiguous()) is None
    assert ctx.info('fisher_analytic_pass') == -1
    with pytest.raises(NotImplementedError, match='Kaiser'):
        fisher.evaluate(centres)
    auto, finite = _fisher(like, 'auto').evaluate(centres), _fisher(like, 'finite').evaluate(centres)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(auto, finite))


def test_profiler_with_analytic_derivatives():
    """An MLP likelihood whose data is the ORACLE's theory at theta*, the solved parameters' priors centred there (zero: their values at theta*), four starts: the best
    fit within 100 x xtol errors of theta* (the rule of tests/test_gpu_fisher_analytic.py::test_profiler_with_analytic_derivatives: margin over the stopping rule), in no
    more iterations than the finite run."""
    from desilike_amd.theories.galaxy_clustering import LPTVelocileptorsTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    from desilike_amd.profilers import GaussNewtonProfiler
    g, like0, pt, theory0, solved = make_mlp_likelihood(marg=True, seed=5, hidden=(24, 40), activation='tanh')
    fisher0 = _fisher(like0)
    names = fisher0.varied_params.names()
    truth = np.array([0. if name in solved else {'qpar': 1.01, 'qper': 0.995, 'dm': 0.01}.get(name, float(like0.all_params[name].value)) for name in names])
    for name, value in zip(names, truth):
        prior = like0.all_params[name].prior
        if prior.dist == 'norm': truth[names.index(name)] = prior.loc          # (every Gaussian prior centred at theta*: the posterior maximum is theta* itself)
    oracle = EmulatedJacobianOracle(like0, pt, theory0, EMU_PARAMS, 'lpt', names)
    data = oracle.jacobian(truth)[0]
    theory = LPTVelocileptorsTracerPowerSpectrumMultipoles(pt=pt, tracer='ELG')
    for name in solved: theory.init.params[name].update(derived='.marg')
    theory.init.params['sn4p'].update(fixed=True, value=0.3)
    obs = TracerPowerSpectrumMultipolesObservable(data=data, kedges=np.linspace(0.02, 0.2, 37), ells=(0, 2, 4), wmatrix={'resolution': 2}, theory=theory, shotnoise=8e3)
    like = ObservablesGaussianLikelihood(observables=[obs], covariance=g['covariance'])
    xtol = 1e-7
    results = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert _device(_fisher(like), truth[None, :]) is not None
        start = GaussNewtonProfiler(like, seed=11)._get_start_points(4)
        for derivatives in ('analytic', 'finite'):
            profiler = GaussNewtonProfiler(like, seed=11, derivatives=derivatives)
            assert profiler.fisher.varied_params.names() == names
            profiles = profiler.maximize(start=start, xtol=xtol)
            index = profiles.argmax()
            best = np.array([profiles.bestfit[name][index] for name in names])
            errors = np.array([profiles.error[name][index] for name in names])
            results[derivatives] = ((np.abs(best - truth) / errors).max(), np.asarray(profiles.attrs['iterations']))
            print('profiler {}: distance to theta* = {:.3e} errors, iterations {}'.format(derivatives, results[derivatives][0], results[derivatives][1]))
    assert results['analytic'][0] <= 100. * xtol, results['analytic'][0]
    assert results['analytic'][1].sum() <= results['finite'][1].sum(), (results['analytic'][1], results['finite'][1])          # (over the four starts)
