"""GPU (-m gpu): the analytic log-posterior gradient (dl_fullshape_grad_kernel + dl_grad_finalize_kernel) and the analytic Jacobian / Fisher path (dl_fullshape_jac_kernel ->
window GEMM -> dl_fisher_kernel<TILES, true>) over the shapes the two benchmark configurations do not reach: one to five multipoles (both template instantiations, with and
without the monopole), the AP modes, the three spline passes (dm / dn sampled or fixed), the fixed template, cross-spectra, mu node counts that are no multiple of four, the
three wavenumber-ownership regimes, P = 15 / 16 parameters over five / six observables, a batch across the finalize kernel's block edge.

Reference: the NumPy oracle alone.  Its Jacobian is the Richardson combination of two five-point stencils of its flattheory, J = (16 d(H) - d(2H)) / 15, with its own error
estimate e = |d(H) - d(2H)| / 15, which must stay below a quarter of the tolerance (2.5e-9 of the column's largest entry) for every column a parameter reaches BEFORE the
device's derivatives are looked at.  Then gradient = -J P D + prior gradient, hessian = -J P J^T, offset = -D P D (oracle.fisher_gaussian).
Tolerances, all the project's: 1e-8 of the largest entry per centre (gradient, hessian), 1e-10 (value, offset; Fisher gradient against the log-posterior gradient), 1e-11 / 1e-12
(forward theory vector)."""
import functools

import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

H = 1e-3                # the stencil of tests/test_fisher.py:183-192 (and twice that, for the Richardson step)
REFERENCE_TOL = 2.5e-9  # the reference's own error: a quarter of TOL
TOL = 1e-8              # tests/test_gpu_fisher_analytic.py:70, tests/test_fisher.py:192

DEFAULT = dict(template='shapefit', apmode='qparqper', ells=(0, 2, 4), mu=8, nbins=7, resolution=3, tracers=(None,), dn=False, dm=True, df=True, sn0_prior=None, b1=None,
               n_kin=21, P=None)   # n_kin, P: the shape the case must have to sit on its edge (asserted by check_shape)
ELLS5 = (0, 2, 4, 6, 8)
CASES = {
    # multipoles: NL = 3 with 1 - 2 live rows; no monopole (ell0 < 0: the sn0 column reaches nothing); NL = 5 with 4 live rows; NL = 5 full
    'ells0': dict(ells=(0,)), 'ells02': dict(ells=(0, 2)), 'ells24': dict(ells=(2, 4), sn0_prior=dict(dist='norm', loc=0.05, scale=2.)),
    'ells0246': dict(ells=(0, 2, 4, 6)), 'ells02468': dict(ells=ELLS5),
    # chain rule of the AP modes (dl_fs_grad_chain / dl_fs_jac_chain_matrix), the last one in the <5> kernels
    'qiso': dict(apmode='qiso'), 'qap': dict(apmode='qap'), 'qisoqap': dict(apmode='qisoqap'), 'qisoqap_ells02468': dict(apmode='qisoqap', ells=ELLS5),
    # spline passes: 0, 1, 2; 0, 2 (pass 1 skipped); 0 only
    'dn_free': dict(dn=True), 'dn_only': dict(dn=True, dm=False), 'dm_fixed_dn_fixed': dict(dm=False),
    'fixed_template': dict(template='fixed'),
    'cross': dict(tracers=(('LRG', 'ELG'),), b1=(1.4, 2.3)),
    'mu6': dict(mu=6), 'mu10': dict(mu=10), 'mu7': dict(mu=7), 'mu9': dict(mu=9),   # n_mu % 4 = 2, 2, 3, 1: every remainder of dl_fs_grad_weights_pad
    # wavenumber ownership (a thread owns i0 = tid + KPT 256 t and, KPT = 2, i0 + 256): n_kin = 21, 300, 540, for KPT = 2 (NL = 3) and KPT = 1 (NL = 5)
    'nkin_small': dict(), 'nkin_300': dict(nbins=50, resolution=6, n_kin=300), 'nkin_540': dict(nbins=60, resolution=9, n_kin=540),
    'nkin_300_ells02468': dict(nbins=50, resolution=6, ells=ELLS5, n_kin=300), 'nkin_540_ells02468': dict(nbins=60, resolution=9, ells=ELLS5, n_kin=540),
    # P = 15 (one full 16-row tile with the residual row) and P = 16 (two tiles) over five / six observables sharing dm, dn, qpar, qper (, df)
    'p15': dict(tracers=('BGS', 'LRG', 'ELG', 'QSO', 'LAE'), dn=True, ells=(0, 2), nbins=5, resolution=1, n_kin=5, P=15),
    'p16': dict(tracers=('BGS', 'LRG', 'ELG', 'QSO', 'LAE', 'LBG'), dn=True, df=False, ells=(0, 2), nbins=5, resolution=1, n_kin=5, P=16),
    # forward coverage only (test_forward_five_multipoles, the device-resident ensemble)
    'two_tracers_ells02468': dict(tracers=('LRG', 'ELG'), ells=ELLS5),
}
DERIVATIVE_CASES = [name for name in CASES if name != 'two_tracers_ells02468']
UNREACHED = {'ells24': ['sn0']}   # columns that reach nothing


@functools.lru_cache(maxsize=None)
def build(name):
    """The likelihood of a named case, built once."""
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, FixedPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    case = dict(DEFAULT, **CASES[name])
    if case['template'] == 'fixed': tpl = FixedPowerSpectrumTemplate(z=0.8)
    else:
        tpl = ShapeFitPowerSpectrumTemplate(z=0.8, apmode=case['apmode'])
        if case['dn']: tpl.init.params['dn'].update(fixed=False)
        if not case['dm']: tpl.init.params['dm'].update(fixed=True, value=0.01)
        if not case['df']: tpl.init.params['df'].update(fixed=True)
    kedges = np.linspace(0.01, 0.2, case['nbins'] + 1)
    n = case['nbins'] * len(case['ells'])
    observables = []
    for itracer, tracer in enumerate(case['tracers']):
        kwargs = {} if tracer is None else dict(tracers=list(tracer) if isinstance(tracer, tuple) else tracer)
        theory = KaiserTracerPowerSpectrumMultipoles(template=tpl, mu=case['mu'], **kwargs)
        bias = [name for name in theory.init.params.names() if name.endswith('b1')]
        data = {name: 1.8 - 0.15 * itracer for name in bias}
        if case['b1'] is not None:     # cross-spectrum: two distinct biases, sampled next to their values; the data a little away from them (a non-zero residual everywhere)
            for name, value in zip(bias, case['b1']):
                theory.init.params[name].update(value=value, ref=dict(limits=[value - 0.1, value + 0.1]))
                data[name] = value + 0.05
        if case['sn0_prior'] is not None:
            for name in theory.init.params.names():
                if name.endswith('sn0'): theory.init.params[name].update(prior=case['sn0_prior'])
        if case['template'] != 'fixed' and case['dm']: data['dm'] = 0.01
        observables.append(TracerPowerSpectrumMultipolesObservable(data=data, kedges=kedges, ells=case['ells'], wmatrix={'resolution': case['resolution']},
                                                                   theory=theory, shotnoise=5e3 - 500. * itracer))
    ntot = n * len(observables)
    A = np.random.RandomState(3).standard_normal((ntot, ntot)) * 20.
    like = ObservablesGaussianLikelihood(observables=observables, covariance=A.dot(A.T) + 2e4 * np.eye(ntot))
    like.initialize()
    return like


def check_shape(name, like):
    """The case sits on the edge it is named for: the number of multipoles and mu nodes, the wavenumbers against the 256 / 512 ownership bounds, P against the 16-row tile
    of dl_fisher_kernel.  A change of a default (a nuisance parameter more, another input grid of the window) must fail here, not move the case off its edge silently."""
    case = dict(DEFAULT, **CASES[name])
    for obs in like.observables:
        theory = obs.wmatrix.theory
        assert tuple(theory.ells) == tuple(case['ells']) and np.size(theory.mu) == case['mu'] and np.size(theory.k) == case['n_kin'], (name, theory.ells, np.size(theory.mu), np.size(theory.k))
    assert len(like.observables) == len(case['tracers'])
    if case['P'] is not None: assert len(like.varied_params) == case['P'], (name, like.varied_params.names())
    assert like.precision.shape == (case['nbins'] * len(case['ells']) * len(case['tracers']),) * 2
    regime = {'nkin_small': (1, 255), 'nkin_300': (257, 511), 'nkin_540': (513, 1023)}   # second wavenumber never live / partly live / a second loop trip (KPT = 2)
    for prefix, (low, high) in regime.items():
        if name.startswith(prefix): assert low <= case['n_kin'] <= high, (name, case['n_kin'])
    assert (len(case['ells']) > 3) == ('0246' in name)   # the <5> instantiations (KPT = 1) against the <3> ones (KPT = 2)


def centers_of(like, n=5, seed=17):
    """``n`` centres from the parameters' ``ref`` clipped to the prior, plus the parameters' own values."""
    rng = np.random.RandomState(seed)
    theta = np.column_stack([np.clip(param.ref.sample(size=n, random_state=rng), *param.prior.limits) for param in like.varied_params])
    return np.ascontiguousarray(np.vstack([theta, [param.value for param in like.varied_params]]))


class Oracle(object):
    """The NumPy oracle on the constants of the host-side calculators (bench.oracle_constants, tests/test_gpu_variants.py::oracle_loglike): the concatenated flattheory of
    every observable at one row of the varied parameters.  An observable's vector is kept per set of the inputs it reads: a step of another tracer's parameter costs nothing."""

    def __init__(self, like):
        self.like, self.names = like, like.varied_params.names()
        self.fixed = {param.name: param.value for param in like.all_params if param.name not in self.names}
        self.observables, self.cache = [], {}
        for obs in like.observables:
            wm, theory = obs.wmatrix, obs.wmatrix.theory
            tpl = theory.template
            shapefit = type(tpl).__name__.startswith('ShapeFit')
            c = dict(template='shapefit' if shapefit else 'fixed', k11=tpl.k, pk_dd_fid=tpl.pk_dd_fid, f_fid=tpl.f_fid, kp=getattr(tpl, 'kp', 0.03), a=getattr(tpl, 'a', 0.6), kin=theory.k,
                     mu=theory.mu, wmu_ell=theory.wmu, ellsin=theory.ells, nd=theory.nd, matrix_full=wm.matrix_full, shotnoisein=wm.shotnoisein, shotnoiseout=wm.shotnoiseout, flatdata=obs.flatdata)
            self.observables.append((c, theory._bias_names(), tpl.apmode if shapefit else None))
        self.priors = [dict(dist=param.prior.dist, limits=tuple(param.prior.limits), loc=getattr(param.prior, 'loc', 0.), scale=getattr(param.prior, 'scale', 1.)) for param in like.varied_params]

    def flattheory(self, row):
        p = dict(self.fixed); p.update(zip(self.names, row))
        out = []
        for iobs, (c, bias, apmode) in enumerate(self.observables):
            q = {'b1': (p[bias['b1X']], p[bias['b1Y']]), 'sn0': p[bias['sn0']]}
            if apmode is not None:
                q['qpar'], q['qper'] = orc.ap_qparqper(apmode, 1. / 3., **{name: p[name] for name in ['qpar', 'qper', 'qiso', 'qap'] if name in p})
                q.update(dm=p['dm'], dn=p['dn'], df=p['df'])
            key = (iobs,) + tuple(sorted(q.items()))
            if key not in self.cache: self.cache[key] = orc.fullshape_observable(c, q)['flattheory']
            out.append(self.cache[key])
        return np.concatenate(out)

    def jacobian(self, center):
        """(J_ref [P, n], e_ref [P, n]): Richardson step on the five-point stencils at H and 2 H, and its own error estimate."""
        J, E = [], []
        for ip in range(len(center)):
            def f(x):
                shifted = center.copy(); shifted[ip] += x
                return self.flattheory(shifted)

            def d(h):
                return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)

            dh, d2h = d(H), d(2 * H)
            J.append((16. * dh - d2h) / 15.); E.append(np.abs(dh - d2h) / 15.)
        self.cache.clear()
        return np.array(J), np.array(E)

    def prior_gradient(self, centers):
        out = np.zeros_like(centers)
        for ip, prior in enumerate(self.priors):
            if prior['dist'] == 'norm': out[:, ip] = -(centers[:, ip] - prior['loc']) / (prior['scale'] * prior['scale'])
            else: assert prior['dist'] == 'uniform'
        return out


def reference(name, like):
    """The oracle's value, gradient and Fisher terms at the centres of a case, with the condition on the reference's own error asserted (no device involved)."""
    oracle = Oracle(like)
    centers = centers_of(like)
    flatdata, precision = np.concatenate(like._flatdata_list()), like.precision
    unreached = [oracle.names.index(pname) for pname in UNREACHED.get(name, [])]
    value, gradient, offset, hessian, worst = [], [], [], [], 0.
    for center in centers:
        flat = oracle.flattheory(center)
        J, E = oracle.jacobian(center)
        floor = 16. * np.finfo('f8').eps * np.abs(flat).max() / (12. * H)      # (the rounding floor of tests/test_jacobian.py:94)
        for ip, pname in enumerate(oracle.names):
            scale = np.abs(J[ip]).max()
            if ip in unreached: assert scale <= floor, (name, pname, scale, floor)
            else:
                assert scale > floor, (name, pname, scale, floor)
                worst = max(worst, E[ip].max() / scale)
                assert E[ip].max() <= REFERENCE_TOL * scale, 'reference too coarse: {} d / d {}: e_ref = {:.2e} of scale'.format(name, pname, E[ip].max() / scale)
        o, g, h = orc.fisher_gaussian(flat - flatdata, J, precision)
        offset.append(o); gradient.append(g); hessian.append(h)
        value.append(orc.gaussian_loglikelihood(flat, flatdata, precision)[0] + orc.logprior(center, oracle.priors))
    print('{}: reference error e_ref <= {:.2e} of scale over the reached columns'.format(name, worst))
    prior_gradient = oracle.prior_gradient(centers)
    return dict(oracle=oracle, centers=centers, value=np.array(value), fisher_gradient=np.array(gradient), gradient=np.array(gradient) + prior_gradient, offset=np.array(offset),
                hessian=np.array(hessian), prior_gradient=prior_gradient, unreached=unreached, e_ref=worst)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Likelihood, reference and the device's evaluations (each taken twice) of a case, computed once for the tests that share them."""
    import torch
    like = build(name)
    check_shape(name, like)
    ref = reference(name, like)               # (asserts the condition on the reference before anything below)
    ctx = like._get_context()
    device = torch.device('cuda', ctx.device)
    t = torch.as_tensor(ref['centers'], dtype=torch.float64, device=device).contiguous()
    runs = []
    for _ in range(2):
        status = torch.full((len(t),), -1, dtype=torch.int32, device=device)
        grad = ctx.eval_logposterior_grad(t, status=status)
        fisher = ctx.eval_fisher_analytic(t)
        torch.cuda.synchronize(device)
        # inside the scope of dl_fs_grad_applicable: Kaiser, fixed / ShapeFit template on uniform knots, no damping -- every case of this file
        assert grad is not None and fisher is not None, name
        runs.append(dict(value=grad[0].cpu().numpy(), gradient=grad[1].cpu().numpy(), status=status.cpu().numpy(), hessian=fisher[0].cpu().numpy(),
                         fisher_gradient=fisher[1].cpu().numpy(), offset=fisher[2].cpu().numpy()))
    return like, ref, runs


def _relative(a, b):
    """max |a - b| per centre, in units of the largest |b| of that centre."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)


@pytest.mark.parametrize('name', DERIVATIVE_CASES)
def test_logposterior_gradient_vs_oracle(name):
    """(a) Context.eval_logposterior_grad: value (1e-10, relative above 1), gradient (1e-8 of the largest component per centre), status."""
    like, ref, (dev, _) = _case(name)
    assert (dev['status'] == 0).all(), dev['status']
    verr = np.abs(dev['value'] - ref['value']) / np.maximum(1., np.abs(ref['value']))
    gerr = _relative(dev['gradient'], ref['gradient'])
    print('{}: log-posterior {:.2e}; gradient {:.2e} of the largest component (e_ref {:.2e}); per column {}'.format(
        name, verr.max(), gerr.max(), ref['e_ref'], ', '.join('{} {:.1e}'.format(*item) for item in zip(ref['oracle'].names, np.abs(dev['gradient'] - ref['gradient']).max(axis=0) / np.abs(ref['gradient']).max()))))
    assert (verr <= 1e-10).all(), verr
    assert (gerr <= TOL).all(), gerr
    for ip in ref['unreached']:      # nothing of the likelihood reaches the column: the prior's gradient, exactly
        assert np.array_equal(dev['gradient'][:, ip], ref['prior_gradient'][:, ip]) and (ref['prior_gradient'][:, ip] != 0.).all()


@pytest.mark.parametrize('name', DERIVATIVE_CASES)
def test_fisher_analytic_vs_oracle(name):
    """(b) Context.eval_fisher_analytic: offset (1e-10), gradient = -J P D and hessian = -J P J^T (1e-8 of the largest entry per centre), the hessian exactly symmetric; a
    column that reaches nothing: exactly zero."""
    like, ref, (dev, _) = _case(name)
    gerr, herr = _relative(dev['fisher_gradient'], ref['fisher_gradient']), _relative(dev['hessian'], ref['hessian'])
    oerr = np.abs(dev['offset'] - ref['offset']) / np.maximum(1., np.abs(ref['offset']))
    P = len(ref['oracle'].names)
    blocks = np.abs(dev['hessian'] - ref['hessian']).max(axis=0) / np.abs(ref['hessian']).max()
    print('{}: P = {:d}: offset {:.2e}; gradient {:.2e}, hessian {:.2e} of the largest entry (e_ref {:.2e}); worst hessian entry at {}'.format(
        name, P, oerr.max(), gerr.max(), herr.max(), ref['e_ref'], [ref['oracle'].names[i] for i in np.unravel_index(blocks.argmax(), blocks.shape)]))
    assert np.allclose(dev['offset'], ref['offset'], rtol=1e-10, atol=1e-10), oerr
    assert (gerr <= TOL).all(), gerr
    assert (herr <= TOL).all(), herr
    assert all(np.array_equal(h, h.T) for h in dev['hessian'])
    for ip in ref['unreached']:
        assert (dev['fisher_gradient'][:, ip] == 0.).all() and (dev['hessian'][:, ip, :] == 0.).all() and (dev['hessian'][:, :, ip] == 0.).all()


@pytest.mark.parametrize('name', DERIVATIVE_CASES)
def test_gradient_consistency_and_determinism(name):
    """(c) the Fisher gradient is the log-posterior gradient minus the prior's (1e-10 of the largest component); (d) two calls give the same bits."""
    like, ref, (dev, again) = _case(name)
    err = _relative(dev['fisher_gradient'], dev['gradient'] - ref['prior_gradient'])
    print('{}: Fisher gradient vs log-posterior gradient: {:.2e}'.format(name, err.max()))
    assert (err <= 1e-10).all(), err
    for key in dev: assert np.array_equal(dev[key], again[key]), (name, key)


def test_finalize_block_edge_b65():
    """dl_grad_finalize_kernel across its 64-thread block: B = 65 with row 64 (the only row of the second block) outside a uniform prior and row 3 NaN in one column:
    -inf and a zero gradient there, the status of eval_logposterior, and the other rows what they are in a batch without the bad rows."""
    import torch
    like, ref, runs = _case('ells02')
    ctx = like._get_context()
    device = torch.device('cuda', ctx.device)
    names = ref['oracle'].names
    rng = np.random.RandomState(65)
    clean = ref['centers'][rng.randint(len(ref['centers']), size=65)] + 1e-3 * rng.uniform(-1., 1., size=(65, len(names)))
    clean[:6] = ref['centers']
    bad = clean.copy()
    assert like.varied_params['qpar'].prior.dist == 'uniform'
    bad[64, names.index('qpar')] = 5.
    bad[3, names.index('df')] = np.nan
    out = {}
    for key, theta in [('clean', clean), ('bad', bad)]:
        t = torch.as_tensor(theta, dtype=torch.float64, device=device).contiguous()
        status, status_ref = torch.full((65,), -1, dtype=torch.int32, device=device), torch.full((65,), -1, dtype=torch.int32, device=device)
        value, grad = ctx.eval_logposterior_grad(t, status=status)
        value_ref = torch.empty(65, dtype=torch.float64, device=device)
        ctx.eval_logposterior(t, value_ref, status=status_ref)
        torch.cuda.synchronize(device)
        out[key] = [a.cpu().numpy() for a in (value, grad, status, value_ref, status_ref)]
    value, grad, status, value_ref, status_ref = out['bad']
    cvalue, cgrad, cstatus = out['clean'][:3]
    good = np.ones(65, dtype='?'); good[[3, 64]] = False
    assert (cstatus == 0).all() and np.array_equal(status, status_ref) and (status[good] == 0).all() and (status[~good] != 0).all(), status
    assert np.isneginf(value[~good]).all() and np.isneginf(value_ref[~good]).all() and (grad[~good] == 0.).all()
    verr = np.abs(value[good] - cvalue[good]).max() / np.abs(cvalue).max()
    gerr = np.abs(grad[good] - cgrad[good]).max() / np.abs(cgrad).max()
    print('b65: neighbours of the bad rows: value {:.2e}, gradient {:.2e} of the largest'.format(verr, gerr))
    assert verr <= 1e-11 and gerr <= 1e-11
    assert (np.abs(value[good] - value_ref[good]) <= 1e-10 * np.maximum(1., np.abs(value_ref[good]))).all()
    # and the six centres of the case inside this batch against the oracle
    assert (_relative(cgrad[:6], ref['gradient']) <= TOL).all()


@pytest.mark.parametrize('name', ['ells0246', 'ells02468', 'two_tracers_ells02468'])
def test_forward_five_multipoles(name):
    """The <5> instantiations of the forward kernels (the derivative checks rest on them): the theory vector and the log-likelihood against the oracle at B = 7 (the
    512-thread form; two observables: the merged launch) and B = 2100 (the 256-thread form, the split-K side of the chi2 switch; two observables: the dense merged launch),
    the same rows in both batches."""
    like = build(name)
    oracle = Oracle(like)
    rng = np.random.RandomState(29)
    theta = np.column_stack([np.clip(param.ref.sample(size=2100, random_state=rng), *param.prior.limits) for param in like.varied_params])
    ctx = like._get_context()
    flatdata = np.concatenate(like._flatdata_list())
    small, big = ctx.eval_batch_host(theta[:7], return_flattheory=True), ctx.eval_batch_host(theta, return_flattheory=True)
    worst = 0.
    for out, rows in [(small, range(7)), (big, [0, 6, 7, 1000, 2047, 2048, 2099])]:
        assert (out[2] == 0).all()
        for i in rows:
            ref_flat = oracle.flattheory(theta[i])
            ref_ll = orc.gaussian_loglikelihood(ref_flat, flatdata, like.precision)[0]
            worst = max(worst, np.abs(out[3][i] - ref_flat).max() / np.abs(ref_flat).max())
            assert np.allclose(out[3][i], ref_flat, rtol=1e-11, atol=1e-12 * np.abs(ref_flat).max()), (name, i)
            assert abs(out[0][i] - ref_ll) <= 1e-10 * max(1., abs(ref_ll)), (name, i, out[0][i], ref_ll)
    print('{}: theory vector {:.2e} of the largest entry'.format(name, worst))
    assert np.allclose(big[0][:7], small[0], rtol=1e-10, atol=1e-10) and np.array_equal(big[1][:7], small[1])
    assert np.allclose(big[3][:7], small[3], rtol=1e-10, atol=1e-12 * np.abs(small[3]).max())


def test_device_ensemble_five_multipoles():
    """dl_fullshape_ens_kernel<5>: the device-resident ensemble on the two-tracer l = 0 ... 8 likelihood against the NumPy driver fed by eval_logposterior, bit for bit."""
    from test_gpu_sampler import _check_against_numpy_driver
    _check_against_numpy_driver(build('two_tracers_ells02468'), 64, 3)
