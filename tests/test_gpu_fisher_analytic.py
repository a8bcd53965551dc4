"""GPU (-m gpu): dl_eval_fisher_analytic -- the Fisher algebra on exact derivative rows (csrc/dl_fullshape_jac.h -> window GEMM -> MFMA Gram product), through
``Context.eval_fisher_analytic``, ``Fisher(method=...)`` and ``GaussNewtonProfiler(derivatives=...)``: against the NumPy oracle's Jacobian (five-point stencil),
the finite-difference path, the analytic log-posterior gradient, and on the scope boundary."""
import functools

import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

H = 1e-3          # the stencil of tests/test_fisher.py:183-192


def _centers(g, like, n):
    rnames = [str(name) for name in g['names']]
    return np.ascontiguousarray(g['theta'][:n, [rnames.index(name) for name in like.varied_params.names()]])


def _oracle_flattheory(g, names, row):
    from golden_utils import observable_constants
    p = dict(zip(names, row))
    out, iobs = [], 0
    while 'obs{:d}'.format(iobs) in g:
        c = observable_constants(g, iobs)
        prefix = str(c['tracer']) + '.' if str(c.get('tracer', '')) else ''
        out.append(orc.fullshape_observable(c, dict(p, b1=(p[prefix + 'b1'],) * 2, sn0=p[prefix + 'sn0']))['flattheory'])
        iobs += 1
    return np.concatenate(out)


def _oracle_fisher(g, like, centers):
    """(offset, gradient, hessian) from the oracle: J by the five-point stencil of its flattheory, then fisher.py:739-748."""
    names = like.varied_params.names()
    flatdata = np.concatenate(like._flatdata_list())
    out = []
    for center in centers:
        rows = []
        for ip in range(len(center)):
            def f(x):
                shifted = center.copy(); shifted[ip] += x
                return _oracle_flattheory(g, names, shifted)
            rows.append((-f(2 * H) + 8 * f(H) - 8 * f(-H) + f(-2 * H)) / (12 * H))
        out.append(orc.fisher_gaussian(_oracle_flattheory(g, names, center) - flatdata, np.array(rows), like.precision))
    return [np.array([o[i] for o in out]) for i in range(3)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Likelihood, centres and the three evaluations of a configuration, computed once for the tests that share them."""
    from test_host_api import make_cfg2, make_cfg5
    from desilike_amd.fisher import Fisher
    g, like = make_cfg2() if name == 'cfg2' else make_cfg5()
    centers = _centers(g, like, 6 if name == 'cfg2' else 3)
    analytic = Fisher(like, method='analytic').evaluate(centers)
    finite = Fisher(like, method='finite').evaluate(centers)
    return g, like, centers, analytic, finite, _oracle_fisher(g, like, centers)


@pytest.mark.parametrize('name', ['cfg2', 'cfg5'])
def test_fisher_analytic_vs_oracle_jacobian(name):
    """hessian = -J P J^T and gradient = -J P D with the oracle's J, 1e-8 of the largest entry; the offset is dl_eval_fisher's (the same residual).  cfg5: the shared
    columns (qpar, qper, dm, df) carry both observables' contributions and the namespaced b1 / sn0 rows are zero in the other observable's block -- the cross terms of
    the Hessian say so."""
    g, like, centers, (offset, gradient, hessian), finite, (roffset, rgradient, rhessian) = _case(name)
    for ib in range(len(centers)):
        herr, gerr = np.abs(hessian[ib] - rhessian[ib]).max() / np.abs(rhessian[ib]).max(), np.abs(gradient[ib] - rgradient[ib]).max() / np.abs(rgradient[ib]).max()
        print('{} centre {:d}: hessian {:.2e}, gradient {:.2e} of the largest entry'.format(name, ib, herr, gerr))
        assert herr <= 1e-8 and gerr <= 1e-8, (ib, herr, gerr)
        assert np.array_equal(hessian[ib], hessian[ib].T)
    assert (np.abs(offset - finite[0]) <= 1e-12 * np.abs(finite[0])).all(), np.abs(offset / finite[0] - 1.).max()
    assert np.allclose(offset, roffset, rtol=1e-10, atol=1e-10)


def test_fisher_analytic_vs_finite_cfg2():
    g, like, centers, analytic, finite, ref = _case('cfg2')
    for a, f in zip(analytic[1:], finite[1:]):
        assert np.allclose(a, f, rtol=1e-3, atol=1e-5 * np.abs(a).max())        # (the bound of tests/test_fisher.py:195: central differences with the parameters' own steps)


@pytest.mark.parametrize('name', ['cfg2', 'cfg5'])
def test_fisher_gradient_is_the_loglikelihood_gradient(name):
    """Inside the priors the Fisher gradient of the likelihood term is d logL / d theta = dl_eval_logposterior_grad minus the prior gradient (uniform: 0, norm: explicit)."""
    from desilike_amd.fisher import logposterior_value_and_grad
    g, like, centers, (offset, gradient, hessian), finite, ref = _case(name)
    value, grad = logposterior_value_and_grad(like, centers, method='analytic')
    inside = np.isfinite(value)
    assert inside.sum() >= 2
    prior_gradient = np.zeros_like(centers)
    for ip, param in enumerate(like.varied_params):
        if param.prior.dist == 'norm': prior_gradient[:, ip] = -(centers[:, ip] - param.prior.loc) / param.prior.scale**2
        else: assert param.prior.dist == 'uniform'
    err = np.abs(gradient - (grad - prior_gradient))[inside].max(axis=1) / np.abs(gradient[inside]).max(axis=1)
    print('{}: Fisher gradient vs analytic log-posterior gradient: {}'.format(name, err))
    assert (err <= 1e-10).all()


def test_plumbing():
    """B = 0, 1, 17, a batch larger than one pass; two calls give the same bits; NULL outputs."""
    import torch
    g, like, centers, analytic, finite, ref = _case('cfg2')
    ctx = like._get_context()
    device = torch.device('cuda', ctx.device)
    P = centers.shape[1]
    hessian, gradient, offset = ctx.eval_fisher_analytic(torch.empty((0, P), dtype=torch.float64, device=device))
    assert hessian.shape == (0, P, P) and gradient.shape == (0, P) and offset.shape == (0,)
    rng = np.random.RandomState(7)
    B = 2048 + 17                                  # (passes are at most 2048 centres: 1856 at this shape)
    big = centers[rng.randint(len(centers), size=B)] + 1e-3 * rng.uniform(-1., 1., size=(B, P))
    t = torch.as_tensor(big, device=device).contiguous()
    first = [a.clone() for a in ctx.eval_fisher_analytic(t)]
    second = ctx.eval_fisher_analytic(t)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(bool(torch.isfinite(a).all()) for a in first)
    # a small batch against the same centres inside the large one, in the first pass and in the second.  Not the same bits: the split of K in the window GEMM depends on
    # the number of rows, so the K_pad-term sums are taken in another order -- K_pad eps ~ 1e-13 of a row entry; 1e-11 of the largest entry leaves two digits
    def close(a, b):
        return bool((a - b).abs().max() <= 1e-11 * b.abs().max())

    for n in (1, 17):
        for start in (0, 2048):
            part = ctx.eval_fisher_analytic(t[start:start + n].contiguous())
            assert all(a.shape[0] == n and close(a, b[start:start + n]) for a, b in zip(part, first)), (n, start)
    full = [a.clone() for a in ctx.eval_fisher_analytic(t[:17].contiguous())]       # (the same batch size: the same bits)
    only_h = ctx.eval_fisher_analytic(t[:17].contiguous(), gradient=False, offset=False)
    only_g = ctx.eval_fisher_analytic(t[:17].contiguous(), hessian=False, offset=False)
    none = ctx.eval_fisher_analytic(t[:17].contiguous(), hessian=False, gradient=False, offset=False)
    torch.cuda.synchronize()
    assert only_h[1] is None and only_h[2] is None and torch.equal(only_h[0], full[0]) and torch.equal(only_g[1], full[1]) and none == (None, None, None)
    # a NaN input: NaN outputs for that centre (dl_eval_fisher's centre row does the same), the others as before
    bad = big[:3].copy(); bad[1, 2] = np.nan
    out = [a.cpu().numpy() for a in ctx.eval_fisher_analytic(torch.as_tensor(bad, device=device).contiguous())]
    # (offset and gradient carry the NaN residual; so does every Hessian entry but (sn0, sn0): that derivative row is the constant 1 / nd, whatever theta holds)
    isn = like.varied_params.names().index('sn0')
    expected_nan = np.ones((P, P), dtype='?'); expected_nan[isn, isn] = False
    assert np.isnan(out[2][1]) and np.isnan(out[1][1]).all() and np.isnan(out[0][1][expected_nan]).all() and all(np.allclose(a[[0, 2]], b[[0, 2]].cpu().numpy(), rtol=0., atol=1e-11 * float(b[[0, 2]].abs().max())) for a, b in zip(out, first))


def test_defaults_do_not_move():
    from desilike_amd.fisher import Fisher
    g, like, centers, analytic, finite, ref = _case('cfg2')
    default = Fisher(like).evaluate(centers)
    assert all(np.array_equal(a, b) for a, b in zip(default, finite))
    auto = Fisher(like, method='auto').evaluate(centers)
    assert all(np.array_equal(a, b) for a, b in zip(auto, analytic))
    with pytest.raises(ValueError):
        Fisher(like, method='exact')


def _out_of_scope_likelihoods():
    from test_host_api import make_cfg4
    from test_gpu_variants import build
    return {'bao_pk': make_cfg4('pk')[1], 'cubic_transform': build(template='shapefit', transform='cubic', covariance='diag', ells=(0, 2))[0],
            'sigmapar_sampled': build(template='shapefit', damping=True)[0]}


@pytest.mark.parametrize('name', ['bao_pk', 'cubic_transform', 'sigmapar_sampled'])
def test_out_of_scope(name):
    import torch
    from desilike_amd.fisher import Fisher
    like = _out_of_scope_likelihoods()[name]
    like.initialize()
    ctx = like._get_context()
    rng = np.random.RandomState(1)
    values = np.array([param.value for param in like.varied_params], dtype='f8')
    centers = values * (1. + 1e-3 * rng.uniform(-1., 1., size=(2, values.size)))          # (next to the parameters' own values: the likelihood is finite there)
    assert ctx.eval_fisher_analytic(torch.as_tensor(centers, device=torch.device('cuda', ctx.device)).contiguous()) is None
    with pytest.raises(NotImplementedError, match='Kaiser'):
        Fisher(like, method='analytic').evaluate(centers)
    auto, finite = Fisher(like, method='auto').evaluate(centers), Fisher(like, method='finite').evaluate(centers)
    # (bit for bit; equal_nan: central differences of a column can be NaN on these configurations -- sn0 under the cubic transform -- in both calls alike)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(auto, finite)) and np.isfinite(finite[0]).all()


def test_profiler_with_analytic_derivatives():
    """config 2 with the data replaced by the ORACLE's theory vector at theta* (no noise; sn0* = 0, the centre of its Gaussian prior, so that the posterior maximum is
    theta* itself).  With zero residual Gauss-Newton is Newton and Levenberg-Marquardt stops when a step is below xtol in units of the errors: the best fit sits
    within 100 x xtol errors of theta* (the factor 100 is margin over the stopping rule, not a measurement)."""
    from golden_utils import load_golden
    from test_host_api import make_cfg2
    from desilike_amd.profilers import GaussNewtonProfiler
    g = load_golden('cfg2_shapefit_window')
    names = [str(n) for n in g['names']]
    truth = np.array([1.01, 0.995, 0.01, 1.02, 1.9, 0.])
    _, like = make_cfg2(data=_oracle_flattheory(g, names, truth))
    assert like.varied_params.names() == names
    xtol = 1e-7
    start = GaussNewtonProfiler(like, seed=11)._get_start_points(4)
    results = {}
    for derivatives in ('analytic', 'finite'):
        profiler = GaussNewtonProfiler(like, seed=11, derivatives=derivatives)
        profiles = profiler.maximize(start=start, xtol=xtol)
        index = profiles.argmax()
        best = np.array([profiles.bestfit[name][index] for name in names])
        errors = np.array([profiles.error[name][index] for name in names])
        results[derivatives] = (best, (np.abs(best - truth) / errors).max(), profiles.attrs['iterations'][index])
    # both best fits re-evaluated with the analytic gradient
    exact = GaussNewtonProfiler(like, seed=11, derivatives='analytic')
    norms = {}
    for derivatives, (best, distance, iterations) in results.items():
        f, gradient, curvature = exact._evaluate(best[None, :])
        norms[derivatives] = float(np.abs(gradient[0] / np.sqrt(np.diag(curvature[0]))).max())
        print('profiler {}: distance to theta* = {:.3e} errors, gradient_norm (analytic gradient) = {:.3e}, {:d} iterations'.format(derivatives, distance, norms[derivatives], iterations))
    assert results['analytic'][1] <= 100. * xtol, results['analytic'][1]
    assert norms['analytic'] <= norms['finite'], norms
