"""The cases of the solved-count sweep (tests/test_gpu_marg_counts.py on the GPU, their input conditions in tests/test_marg_reference.py on the CPU).  Residual route: EFT-like Kaiser
tracers -- per tracer the counter terms ct{0,2,4}_2 (point-dependent derivative rows, var_slot >= 0) and the stochastic terms sn{0,2,4}_2 (constant rows) -- with a dense window and a
dense cross-covariance; the first ``n_s`` of the ordered list of linear parameters are solved, the others fixed at 0.  Gram route (second half): one emulated velocileptors observable.
Every case carries its data (the oracle's theory at a drawn point + one noise draw of the covariance), 8 rows of theta and, from the oracle's theory chain, Delta(x0) and T of
those rows.  Everything here runs on the host (no device)."""
import functools

import numpy as np

from oracle import np_oracle as orc

ELLS3, ELLS2 = (0, 2, 4), (0, 2)
TRACERS = ('LRG', 'ELG', 'QSO')
NROWS = 8      # rows of every case compared with the extended-precision reference


def _layout(n, n_s):
    """[(ells, nk)] per tracer: n data points in all, at least n_s linear parameters (2 per multipole of a tracer)."""
    if n == 57: return [(ELLS3, 19)] if n_s <= 6 else [(ELLS3, 10), (ELLS3, 9)] if n_s <= 12 else [(ELLS3, 7), (ELLS3, 6), (ELLS3, 6)]
    return {20: [(ELLS2, 10)], 120: [(ELLS3, 20)] * 2, 360: [(ELLS3, 40)] * 3, 504: [(ELLS3, 56)] * 3, 512: [(ELLS3, 56), (ELLS3, 56), (ELLS2, 88)], 513: [(ELLS3, 171)]}[n]


# (n, n_s): every count at n = 57 (no multiple of 4); the 512-double floor of the staging region; either side of 48 KB and of 96 KB of LDS; n near and at the limit of 512
CASES = [(57, n_s) for n_s in range(1, 17)] + [(20, 1), (20, 3), (120, 11), (120, 12), (360, 7), (360, 8)] + [(n, n_s) for n in (504, 512) for n_s in (4, 5, 15, 16)]
CASE_IDS = ['n{:d}-ns{:d}'.format(*case) for case in CASES]


# Gaussian prior scales narrowed where the float64 oracle itself would miss condition (b) of tests/test_marg_reference.py (nearly dependent k^2-like rows)
PRIOR_SHRINK = {case: 0.1 for case in [(57, 5), (57, 6), (57, 12), (20, 3), (120, 12), (504, 15)]}


def derivative_rows(flat, f0, n_s):
    """T [n_s, n] of a theory that is exactly linear in the solved parameters, from ``flat(s, step)`` = the theory with solved parameter s moved by ``step`` and f0 = the theory at
    x0.  A unit step would lose digits where a row is small against the theory (the counter-term rows of a shot-noise dominated spectrum: 1e-2 against 1e3): the step is the power
    of two that brings the row to the size of the theory, so that the difference cancels nothing and the division is exact."""
    rows = []
    for s in range(n_s):
        unit = flat(s, 1.) - f0
        step = 2.**np.clip(np.round(np.log2(np.abs(f0).max() / np.abs(unit).max())), 0, 60) if np.abs(unit).max() > 0. else 1.
        rows.append((flat(s, step) - f0) / step)
    return np.array(rows)


def staged_lds_bytes(n, n_s):
    """Dynamic LDS the staged finalize asks for (dl_launch_finalize_marg): four waves of max((1 + n_s) (4 ceil(n / 4) + 4), 512) doubles."""
    return 4 * max((1 + n_s) * (4 * ((n + 3) // 4) + 4), 512) * 8


def expected_branch(n, n_s):
    """The kernel / branch ``dl_launch_finalize_marg`` takes for residual rows (no Gram matrix)."""
    if n_s == 16: return 'serial<false,false>'
    shm = staged_lds_bytes(n, n_s)
    if shm > 96 * 1024: return 'unstaged<true,false>'
    return 'staged<true,true>+attribute' if shm > 48 * 1024 else 'staged<true,true>'


def mask_patterns(n_s, seed):
    """'.marg' masks: all, none ('.best'), only the first, only the last, alternating, a random half (duplicates at small n_s dropped)."""
    rng = np.random.RandomState(seed)
    half = np.zeros(n_s, dtype='?'); half[rng.permutation(n_s)[:max(n_s // 2, 1)]] = True
    first = np.zeros(n_s, dtype='?'); first[0] = True
    last = np.zeros(n_s, dtype='?'); last[-1] = True
    patterns, seen = [], set()
    for name, mask in [('all', np.ones(n_s, dtype='?')), ('none', np.zeros(n_s, dtype='?')), ('first', first), ('last', last), ('alternating', np.arange(n_s) % 2 == 0), ('half', half)]:
        if mask.tobytes() not in seen:
            seen.add(mask.tobytes()); patterns.append((name, mask))
    return patterns


def linear_names(layout):
    return ['{}.{}{:d}_2'.format(tracer, base, ell) for tracer, (ells, nk) in zip(TRACERS, layout) for base in ('ct', 'sn') for ell in ells]


def build(n, n_s, data=None, mask=None):
    """Likelihood of case (n, n_s); ``data`` (list of arrays per tracer; zeros if not given); ``mask``: '.marg' (True) / '.best' per solved parameter, in the order of ``solved`` below."""
    import bench
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, EFTLikeKaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    layout, prior_shrink = _layout(n, n_s), PRIOR_SHRINK.get((n, n_s), 1.)
    assert sum(len(ells) * nk for ells, nk in layout) == n
    rng = np.random.RandomState(1000 * n + n_s)
    solved = linear_names(layout)[:n_s]
    assert len(solved) == n_s
    if mask is None: mask = np.ones(n_s, dtype='?')
    template = ShapeFitPowerSpectrumTemplate(z=0.8, fiducial='synthetic')
    observables, priors = [], {}
    for it, (tracer, (ells, nk)) in enumerate(zip(TRACERS, layout)):
        theory = EFTLikeKaiserTracerPowerSpectrumMultipoles(template=template, tracers=tracer)
        for base in ('ct', 'sn'):
            for ell in ELLS3:
                name = '{}.{}{:d}_2'.format(tracer, base, ell)
                if name in solved:
                    flat = rng.rand() < 0.4
                    loc, scale = float(rng.uniform(0.2, 1.) * rng.choice([-1., 1.])), float(rng.uniform(5., 50.) * prior_shrink)     # Gaussian: loc != x0 = 0
                    priors[name] = (0., np.inf) if flat else (loc, scale)
                    theory.init.params[name].update(derived='.marg' if mask[solved.index(name)] else '.best', prior=dict(dist='uniform') if flat else dict(dist='norm', loc=loc, scale=scale))
                elif ell in ells:
                    theory.init.params[name].update(fixed=True, value=0.)
        kedges = np.linspace(0.02, 0.2, nk + 1)
        kin, full = bench.dense_window(kedges, ells, resolution=2, seed=31 + it)
        observables.append(TracerPowerSpectrumMultipolesObservable(data=np.zeros(len(ells) * nk) if data is None else data[it], kedges=kedges, ells=ells, wmatrix=full, kin=kin, ellsin=ells,
                                                                   theory=theory, shotnoise=[1e4, 4e3, 2e4][it]))
    A = rng.standard_normal((n, n)) * 30.
    like = ObservablesGaussianLikelihood(observables=observables, covariance=A.dot(A.T) + 1e4 * np.eye(n))
    return like, solved, priors


class Case(object):
    """One (n, n_s): data = the oracle's theory at a drawn point x* + one noise draw of the covariance; NROWS rows of theta with, from the oracle's theory chain, Delta(x0) and T."""

    def __init__(self, n, n_s):
        from golden_utils import constants_from_mirror
        self.n, self.n_s = n, n_s
        like, self.solved, self.priors = build(n, n_s)
        like.initialize()
        rng = np.random.RandomState(7000 + 100 * n + n_s)
        self.names = like.varied_params.names()
        assert like.solved_params.names() == self.solved, (like.solved_params.names(), self.solved)
        constants = [constants_from_mirror(obs) for obs in like.observables]
        self.constants, self.covariance = constants, like.covariance
        xstar = np.array([np.clip(param.ref.sample(random_state=rng), *param.prior.limits) for param in like.varied_params], dtype='f8').ravel()
        solved_star = dict(zip(self.solved, rng.standard_normal(n_s)))
        noise = rng.multivariate_normal(np.zeros(n), like.covariance)
        self.flatdata = self.flattheory(xstar, solved_star) + noise
        sizes = np.cumsum([0] + [len(c['flatdata']) for c in constants])
        self.data = [self.flatdata[lo:hi] for lo, hi in zip(sizes[:-1], sizes[1:])]
        self.x0 = np.zeros(n_s)
        self.prior_loc, self.prior_scale = (np.array([self.priors[name][i] for name in self.solved]) for i in range(2))
        # rows drawn like a sampler's start, pulled towards x* (a third of the way out): chi2(x0) stays of the order of n, see condition (a) in tests/test_marg_reference.py
        draws = np.column_stack([np.clip(param.ref.sample(size=NROWS, random_state=rng), *param.prior.limits) for param in like.varied_params])
        self.theta = xstar + (draws - xstar) / 3.
        self.varied_priors = [dict(dist=param.prior.dist, limits=tuple(param.prior.limits), loc=getattr(param.prior, 'loc', 0.), scale=getattr(param.prior, 'scale', 1.)) for param in like.varied_params]
        self.precision = like.precision
        self.delta, self.T = [], []
        for row in self.theta:
            f0 = self.flattheory(row, {})
            self.T.append(derivative_rows(lambda s, step: self.flattheory(row, {self.solved[s]: step}), f0, n_s))
            self.delta.append(f0 - self.flatdata)
        self.n_var = sum('.ct' in name for name in self.solved)      # point-dependent derivative rows: 1 + n_var rows per point go through the window GEMM

    def flattheory(self, row, solved):
        p = dict(zip(self.names, row))
        out = []
        for tracer, c in zip(TRACERS, self.constants):
            q = {name: p[name] for name in ['qpar', 'qper', 'dm', 'df'] if name in p}
            q['b1'] = (p[tracer + '.b1'], p[tracer + '.b1'])
            q['sn0'] = p.get(tracer + '.sn0', 0.)
            q['ct'] = [2. * solved.get('{}.{}'.format(tracer, name), 0.) for name in c['ct_params']]      # auto-spectrum: both tracer inputs of a term are the same parameter
            q['sn'] = [q['sn0'] if name == 'sn0' else solved.get('{}.{}'.format(tracer, name), 0.) for name in c['sn_params']]
            out.append(orc.fullshape_observable(c, q)['flattheory'])
        return np.concatenate(out)

    def likelihood(self, mask):
        return build(self.n, self.n_s, data=self.data, mask=mask)[0]

    def logprior_varied(self, rows):
        return orc.logprior(np.asarray(rows), self.varied_priors)


@functools.lru_cache(maxsize=4)
def get_case(n, n_s):
    return Case(n, n_s)


# ---- Gram route: one emulated observable (N_pad = 128), the Gram matrix of [d~; T~] comes out of the feature GEMM ----------------------------------------------------
# The linear inputs of an emulated velocileptors theory are its counter and stochastic terms: six in the 'physical' basis (alpha6 is f^2 alpha4p there), seven in the
# 'standard' basis.  Pass-through columns of the window (systematic templates) switch the feature path off (dl_create: n_pass != 0), several observables too.
GRAM_LINEAR = {'physical': ['alpha0p', 'alpha2p', 'alpha4p', 'sn0p', 'sn2p', 'sn4p'], 'standard': ['alpha0', 'alpha2', 'alpha4', 'alpha6', 'sn0', 'sn2', 'sn4']}
GRAM_CASES = [('mlp', 'physical', count) for count in range(1, 7)] + [('mlp', 'standard', 7)] + [('taylor', 'physical', count) for count in range(1, 7)]
GRAM_CASE_IDS = ['{}-{}-ns{:d}'.format(*case) for case in GRAM_CASES]
_BIAS = {'physical': ['b1p', 'b2p', 'bsp', 'b3p'], 'standard': ['b1', 'b2', 'bs', 'b3']}


class GramCase(object):
    """One (engine, prior basis, count): ``make_mlp_likelihood`` of tests/test_gpu_emulator.py or the Taylor variant ``make_cfg3`` with the first ``count`` linear parameters solved."""

    def __init__(self, kind, basis, count):
        from golden_utils import load_golden
        self.kind, self.basis, self.n_s = kind, basis, count
        self.solved = GRAM_LINEAR[basis][:count]
        rng = np.random.RandomState(500 + 10 * count + len(kind))
        self.priors = {}
        for name in self.solved:
            flat = rng.rand() < 0.4
            self.priors[name] = (0., np.inf) if flat else (float(rng.uniform(0.2, 1.) * rng.choice([-1., 1.])), float(rng.uniform(2., 12.)))
        like = self.likelihood(np.ones(count, dtype='?'))
        like.initialize()
        self.theory = self._built_theory
        assert like.solved_params.names() == self.solved, (like.solved_params.names(), self.solved)
        self.names = like.varied_params.names()
        self.g = load_golden('cfg3_velocileptors_table')
        self.n = len(like.flatdata)
        self.precision, self.covariance = like.precision, self.g['covariance']
        self.x0 = np.array([param.value for param in like.solved_params], dtype='f8')
        self.values = {param.name: param.value for param in like.all_params if param.value is not None}
        self.prior_loc, self.prior_scale = (np.array([self.priors[name][i] for name in self.solved]) for i in range(2))
        self.varied_priors = [dict(dist=param.prior.dist, limits=tuple(param.prior.limits), loc=getattr(param.prior, 'loc', 0.), scale=getattr(param.prior, 'scale', 1.)) for param in like.varied_params]
        xstar = np.array([np.clip(param.ref.sample(random_state=rng), *param.prior.limits) for param in like.varied_params], dtype='f8').ravel()
        solved_star = dict(zip(self.solved, self.x0 + 0.1 * rng.standard_normal(count)))
        self._like = like
        self.flatdata = self.flattheory(xstar, solved_star) + rng.multivariate_normal(np.zeros(self.n), self.covariance)
        draws = np.column_stack([np.clip(param.ref.sample(size=NROWS, random_state=rng), *param.prior.limits) for param in like.varied_params])
        self.theta = xstar + (draws - xstar) / 20.     # (the counter terms that stay sampled move the theory by many sigma over their ref distributions: condition (a))
        self.delta, self.T = [], []
        for row in self.theta:
            f0 = self.flattheory(row, dict(zip(self.solved, self.x0)))
            self.T.append(derivative_rows(lambda s, step: self.flattheory(row, dict(zip(self.solved, self.x0 + step * np.eye(count)[s]))), f0, count))
            self.delta.append(f0 - self.flatdata)

    def likelihood(self, mask):
        flags = {name: '.marg' if m else '.best' for name, m in zip(self.solved, mask)}
        if self.kind == 'mlp':
            from test_gpu_emulator import make_mlp_likelihood
            _, like, self.pt, theory, _ = make_mlp_likelihood(marg=True, derived=flags, prior_basis=self.basis)
            params = theory.init.params
        else:
            from test_host_api import make_cfg3
            like = make_cfg3(marg=False)[1]
            like.initialize()
            theory = like.observables[0].wmatrix.theory
            params = theory.init.params
            for name in self.solved: params[name].update(derived=flags[name])
        for name in self.solved:
            loc, scale = self.priors[name]
            params[name].update(fixed=False, prior=dict(dist='uniform') if np.isinf(scale) else dict(dist='norm', loc=loc, scale=scale))
        if self.kind != 'mlp': like._invalidate()
        self._built_theory = theory
        return like

    def flattheory(self, row, solved):
        """The oracle's chain: emulated tables -> velocileptors combination -> cubic interpolation -> window."""
        from emulator_utils import EMU_PARAMS, taylor_state
        p = dict(self.values); p.update(zip(self.names, row)); p.update(solved)
        xin = np.array([p[name] for name in EMU_PARAMS])
        theory, wm = self.theory, self._like.observables[0].wmatrix
        if self.kind == 'mlp':
            eng = self.pt.engines
            pktable, sigma8, fsigma8 = (orc.mlp_predict(xin, eng[name].xlimits, eng[name].layers, eng[name].activation, eng[name].ylimits) for name in ['pktable', 'sigma8', 'fsigma8'])
            pktable, sigma8, fsigma8 = pktable.reshape(3, -1, 19), sigma8[0], fsigma8[0]
            model, kpt = 'lpt', self.pt.k
        else:
            state = taylor_state(self.g)
            pktable, sigma8, fsigma8 = (orc.taylor_predict(xin, **state[name]) for name in ['pktable', 'sigma8', 'fsigma8'])
            model, kpt = 'rept', self.g['obs0']['kpt']
        params = {name: p.get(name, 0.) for name in _BIAS[self.basis] + GRAM_LINEAR[self.basis]}
        pars = orc.velocileptors_pars(params, sigma8, fsigma8 / sigma8, basis=self.basis, model=model, snd=theory.snd, fsat=theory.fsat, sigv=theory.sigv)
        power = orc.interp1d(theory.k, kpt, orc.tablevel_combine_bias_terms_poles(pktable, pars, nd=theory.nd).T).T
        return orc.window_apply(power, matrix_full=wm.matrix_full, shotnoisein=wm.shotnoisein, shotnoiseout=wm.shotnoiseout)

    def logprior_varied(self, rows):
        return orc.logprior(np.asarray(rows), self.varied_priors)


@functools.lru_cache(maxsize=2)
def get_gram_case(kind, basis, count):
    return GramCase(kind, basis, count)
