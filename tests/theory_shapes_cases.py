"""Shapes of the TNS, BAO and PNG kernels beyond the reference's defaults (tests/test_theory_shapes_cases.py, tests/test_gpu_theory_shapes.py, tests/switch_probe.py): a
table of small likelihoods built through the host mirrors at ragged sizes, and the NumPy oracle's log-likelihood, theory vector and one-loop tables for them.  Test
infrastructure only: numpy, the oracle (oracle/np_oracle.py) and the host mirrors; the device library is never imported here.

Every case is a dict of shape knobs:

    family       'tns' | 'bao' | 'png'
    theory       name of the mirror class (desilike_amd.theories.galaxy_clustering)
    template     'shapefit' | 'bao' | 'phaseshift'
    knots        number of template knots (the class attribute ``_klim`` of a test-side subclass)
    mu           number of projection cosines
    ells         multipoles
    kedges       (kmin, kmax, number of bins) with ``resolution``: n_kin = bins x resolution;  or  s = (smin, smax, number of separations): xi_ell, n_kin = 300
    options      keyword arguments of the theory (fog, mode, model ...)
    free         parameters freed on top of the defaults
    batch        batch size of the GPU test instead of its rotation
    pin          name of the tests/golden/boundary_<pin>.npz whose shape this is (tests/test_theory_shapes_cases.py pins the driver below on it)
    kaiser       a second observable on the Kaiser theory next to the first: (kmax, bins, resolution)

TNS: n11 = int(1.6 n_kin + 0.5) table wavenumbers, K = 10 x knots pairs per wavenumber.  The assembly kernel puts ppw = 3 points into a workgroup from 1536 points and falls
back while ``dl_tns_assemble_doubles(n11, n_in, n_kin, ppw) x 8 = 8 (32 (n11 | 1) + ppw (456 + n_in + n_kin))`` exceeds 80 KB (csrc/dl_tns.h): with three multipoles and
n_kin = 141 (n11 = 226) that is 82592 B at ppw = 3 and 74432 B at ppw = 2 -- case 'tns_lds' (fallback to 2); the correlation-function case 'tns_xi' (n_kin = 300,
n11 = 480: 123136 B of tables alone) falls back to 1.  Both lie within ``dl_create``'s limit of 156 KB at ppw = 1."""
import numpy as np

from oracle import np_oracle as oc

BATCHES = [1, 33, 273, 1025, 1537, 2049]      # rotated over the cases of a family; 1025 and 1537: ppw = 2 and 3 with a remainder

CASES = {
    # ---- TNS: (n_kin, n11, knots, cosines) ------------------------------------------------------------------------------------------------------------------------
    'tns_6_10_12_3': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=12, mu=3, ells=(0, 2), kedges=(0., 0.12, 6), resolution=1, options=dict(fog='lorentzian')),      # K = 120: below the floor of 128 pairs
    'tns_7_11_61_4': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=61, mu=4, ells=(0, 2, 4), kedges=(0., 0.14, 7), resolution=1, options=dict(fog='gaussian')),     # odd n11; K = 610: 14 pairs of padding in the last round
    'tns_9_14_14_16': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=14, mu=16, ells=(0,), kedges=(0.01, 0.19, 9), resolution=1, options=dict(fog='lorentzian'), free=('bs',)),
    'tns_22_35_203_5': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=203, mu=5, ells=(0, 2, 4), kedges=(0., 0.2, 11), resolution=2, options=dict(fog='gaussian'), free=('bs', 'b3')),
    'tns_39_62_130_8': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=130, mu=8, ells=(0, 2), kedges=(0.02, 0.28, 13), resolution=3, options=dict(fog='lorentzian')),
    'tns_5_8_37_2': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=37, mu=2, ells=(0, 2), kedges=(0., 0.1, 5), resolution=1, options=dict(fog='gaussian')),           # K = 370: 14 pairs of padding
    'tns_eft': dict(family='tns', theory='EFTLikeTNSTracerPowerSpectrumMultipoles', knots=37, mu=3, ells=(0, 2, 4), kedges=(0., 0.2, 11), resolution=2, batch=1537),                      # counter terms: 2 points per workgroup, with a remainder
    'tns_xi': dict(family='tns', theory='TNSTracerCorrelationFunctionMultipoles', knots=203, mu=4, ells=(0, 2), s=(32.5, 147.5, 9), options=dict(fog='gaussian'), batch=1537),           # n_kin = 300, n11 = 480: 1 point per workgroup
    'tns_kaiser': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=61, mu=5, ells=(0, 2), kedges=(0., 0.18, 9), resolution=1, options=dict(fog='lorentzian', tracers='LRG'), kaiser=(0.15, 8, 2)),
    'tns_lds': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=37, mu=2, ells=(0, 2, 4), kedges=(0., 0.235, 47), resolution=3, options=dict(fog='lorentzian'), batch=1537),   # n_kin = 141, n11 = 226: ppw 3 -> 2
    'tns_ref': dict(family='tns', theory='TNSTracerPowerSpectrumMultipoles', knots=500, mu=8, ells=(0, 2, 4), kedges=(0., 0.2, 40), resolution=1, options=dict(fog='gaussian'), free=('bs',), shotnoise=1e4, pin='tns', batch=33),
    # ---- BAO: n_kin = bins x resolution ---------------------------------------------------------------------------------------------------------------------------
    'bao_9': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=130, mu=3, ells=(0, 2), kedges=(0.02, 0.29, 3), resolution=3),
    'bao_63': dict(family='bao', theory='ResummedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=257, mu=7, ells=(0, 2), kedges=(0.02, 0.3, 21), resolution=3, options=dict(mode='reciso'), free=('d',), shotnoise=3e3),
    'bao_64': dict(family='bao', theory='FlexibleBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=401, mu=3, ells=(0, 2), kedges=(0.02, 0.3, 16), resolution=4, options=dict(mode='reciso', wiggles='pcs')),
    'bao_65': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=257, mu=7, ells=(0, 2, 4), kedges=(0.02, 0.28, 13), resolution=5, options=dict(mode='recsym', model='fog-damping_move-all'),
                   free=('sigmapar', 'sigmaper')),
    'bao_192': dict(family='bao', theory='ResummedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=130, mu=3, ells=(0, 2), kedges=(0.02, 0.26, 48), resolution=4, options=dict(mode='recsym', model='fog-damping_move-all')),
    'bao_258': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=401, mu=7, ells=(0, 2, 4), kedges=(0.02, 0.278, 43), resolution=6, free=('sigmapar', 'sigmaper')),
    'bao_ps_9': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='phaseshift', knots=130, mu=3, ells=(0, 2), kedges=(0.02, 0.29, 3), resolution=3),
    'bao_ps_258': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='phaseshift', knots=257, mu=7, ells=(0, 2), kedges=(0.02, 0.278, 43), resolution=6, options=dict(mode='reciso')),
    'bao_xi': dict(family='bao', theory='DampedBAOWigglesTracerCorrelationFunctionMultipoles', template='bao', knots=257, mu=3, ells=(0, 2), s=(40., 160., 7), options=dict(mode='reciso')),      # n_kin = 300
    'bao_ref': dict(family='bao', theory='DampedBAOWigglesTracerPowerSpectrumMultipoles', template='bao', knots=2000, mu=10, ells=(0, 2), kedges=(0.02, 0.3, 56), resolution=3, free=('sigmapar', 'sigmaper'), pin='cfg4_pk'),
    # ---- PNG: (n_kin, cosines, knots) -----------------------------------------------------------------------------------------------------------------------------
    'png_7_5_123': dict(family='png', theory='PNGTracerPowerSpectrumMultipoles', knots=123, mu=5, ells=(0, 2), kedges=(0.002, 0.1, 7), resolution=1, options=dict(mode='b-p')),
    'png_99_33_301': dict(family='png', theory='PNGTracerPowerSpectrumMultipoles', knots=301, mu=33, ells=(0, 2), kedges=(0.002, 0.101, 33), resolution=3, options=dict(mode='bphi')),
    'png_26_48_130': dict(family='png', theory='PNGTracerPowerSpectrumMultipoles', knots=130, mu=48, ells=(0, 2, 4), kedges=(0.004, 0.108, 13), resolution=2, options=dict(mode='b-p')),      # DL_PNG_MAX_MU cosines
    'png_velocity': dict(family='png', theory='PNGTracerVelocityPowerSpectrumMultipoles', knots=123, mu=41, ells=(1, 3), kedges=(0.005, 0.105, 5), resolution=3, options=dict(mode='b-p')),   # (its 41 folded trapezoid nodes are the class's own)
    'png_ref': dict(family='png', theory='PNGTracerPowerSpectrumMultipoles', knots=1000, mu=20, ells=(0, 2), kedges=(0.002, 0.102, 25), resolution=2, options=dict(mode='b-p'), shotnoise=1e4, pin='png'),
}

def names(family=None):
    return [name for name, case in CASES.items() if family is None or case['family'] == family]


def batch_size(name):
    """Batch of the GPU test: the case's own, or ``BATCHES`` in turn over the cases of its family."""
    case = CASES[name]
    return case['batch'] if 'batch' in case else BATCHES[names(case['family']).index(name) % len(BATCHES)]


def shape(like):
    """(n_kin, n11 or None, knots, cosines) of the first observable, as the kernels see them."""
    theory = like.observables[0].wmatrix.theory
    n11 = len(theory.k11) if hasattr(theory, 'k11') else None
    return len(theory.kin if hasattr(theory, 'kin') else theory.k), n11, len(theory.template.k), len(theory.mu)


def _subclass(cls, knots):
    """The mirror class with ``knots`` template knots: same name, same everything else."""
    return type(cls.__name__, (cls,), dict(_klim=(cls._klim[0], cls._klim[1], int(knots))))


def _priors(like):
    rows = np.array([param.prior.spec() for param in like.varied_params], dtype='f8').reshape(-1, 5)
    return [dict(dist=['uniform', 'norm'][int(row[0])], limits=(row[1], row[2]), loc=row[3], scale=row[4]) for row in rows]


def build(case, data=None, precision=None):
    """``(like, info)`` of a case (a name of ``CASES`` or a dict): the likelihood through the mirror classes, initialised without the device library.  Data: the oracle's theory
    vector at the parameters' default values plus one seeded draw from the covariance; covariance by the recipe of tests/test_gpu_shapes.py::build, ``A A^T`` of a seeded normal
    matrix plus a diagonal, scaled to 2 % of the theory vector so that chi2 per point is O(1).  ``data`` / ``precision``: taken instead (the pin)."""
    import desilike_amd.theories.galaxy_clustering as tg
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, TracerCorrelationFunctionMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    from desilike_amd.fiducial import SyntheticFiducial
    name = case if isinstance(case, str) else case.get('name', 'case')
    case = dict(CASES[case]) if isinstance(case, str) else dict(case)
    seed = sum(ord(c) for c in name)
    template_name = case.get('template', 'shapefit')
    # the synthetic spectrum; for the one-loop theory scaled up as the reference's fixtures are (tests/golden/make_tns_fixture.py: P(k = 0.1) ~ 1e4, loop terms of several per cent)
    fiducial = SyntheticFiducial(A=2.5e4 * (300. if case['family'] == 'tns' else 1.))
    if template_name == 'shapefit': template = tg.ShapeFitPowerSpectrumTemplate(z=0.5, fiducial=fiducial)
    elif template_name == 'bao': template = tg.BAOPowerSpectrumTemplate(z=0.5, fiducial=fiducial)
    else: template = tg.BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial=fiducial)
    theory = _subclass(getattr(tg, case['theory']), case['knots'])(template=template, mu=case['mu'], **case.get('options', {}))
    for pname in case.get('free', ()): theory.init.params[pname].update(fixed=False)
    if case['family'] == 'bao':
        # broadband terms: the start distribution of the reference (+-100, +-1e-3 for xi_ell) would bury the wiggles under powers of k / kp or s / sp; narrowed to a tenth of the signal at most
        for param in theory.init.params.select(basename='al*'): param.update(ref=dict(limits=[-1e-5, 1e-5] if 's' in case else [-10., 10.]))
    ells = tuple(case['ells'])
    kw = dict(shotnoise=case['shotnoise']) if 'shotnoise' in case else {}
    if 's' in case:
        n = len(ells) * case['s'][2]
        observables = [TracerCorrelationFunctionMultipolesObservable(data=np.zeros(n), s=np.linspace(*case['s']), ells=ells, theory=theory)]
    else:
        n = len(ells) * case['kedges'][2]
        observables = [TracerPowerSpectrumMultipolesObservable(data=np.zeros(n), kedges=np.linspace(case['kedges'][0], case['kedges'][1], case['kedges'][2] + 1), ells=ells,
                                                               wmatrix={'resolution': case['resolution']}, theory=theory, **kw)]
    sizes = [n]
    if 'kaiser' in case:
        kmax, nk, resolution = case['kaiser']
        kaiser = _subclass(tg.KaiserTracerPowerSpectrumMultipoles, case['knots'])(template=template, tracers='ELG')      # (a shared template takes the knots of the theory initialised last)
        observables.append(TracerPowerSpectrumMultipolesObservable(data=np.zeros(3 * nk), kedges=np.linspace(0., kmax, nk + 1), ells=(0, 2, 4), wmatrix={'resolution': resolution}, theory=kaiser,
                                                                   shotnoise=4e3))
        sizes.append(3 * nk)
    for obs in observables: obs.initialize()
    n = sum(sizes)
    if data is None:
        # the parameters' default values: a likelihood with any covariance knows them
        probe = ObservablesGaussianLikelihood(observables=observables, precision=np.ones(n))
        probe.initialize()
        info = dict(name=name, family=case['family'], case=case)
        flat0 = oracle_rows(probe, info, np.array([[param.value for param in probe.varied_params]]))[1][0]
        rng = np.random.RandomState(seed)
        A = rng.standard_normal((n, n))
        # standard deviations of 2 % of every entry's own size (of 5 % of the root mean square at least): the last wavenumbers, where the power is smallest, weigh as much as the first
        sigma = 0.02 * np.maximum(np.abs(flat0), 0.05 * np.sqrt(np.mean(flat0**2)))
        covariance = (A.dot(A.T) + 10. * n * np.eye(n)) * np.outer(sigma, sigma) / (11. * n)
        data = flat0 + np.linalg.cholesky(covariance).dot(rng.standard_normal(n))
        matrix = dict(covariance=covariance)
    else:
        matrix = dict(precision=np.asarray(precision, dtype='f8'))
    start = 0
    for obs, size in zip(observables, sizes):
        obs.flatdata = np.array(data[start:start + size], dtype='f8')
        start += size
    like = ObservablesGaussianLikelihood(observables=observables, **matrix)
    like.initialize()
    return like, dict(name=name, family=case['family'], case=case, n=n, shape=shape(like))


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------------------
def _window(obs, power, drop_last=False):
    """Theory vector of one power-spectrum observable from its multipoles [n_ell, n_kin] (window.py:459-473); ``drop_last``: without the last ``kin`` column."""
    wm = obs.wmatrix
    matrix = wm.matrix_full
    if drop_last:
        matrix = matrix.copy()
        matrix[:, power.shape[1] - 1::power.shape[1]] = 0.
    return oc.window_apply(power, matrix_full=matrix, shotnoisein=wm.shotnoisein, shotnoiseout=wm.shotnoiseout)


def _corr(theory, power, drop_last=False):
    """xi_ell at the observable's separations from the multipoles on the theory's ``kin`` (tgc/base.py:62-77, 127-136)."""
    if drop_last: power = np.concatenate([power[:, :-1], np.zeros((power.shape[0], 1))], axis=1)
    return np.ravel(oc.get_corr(power, theory.kin, theory.s, theory.ells))


def _tns_point(theory, p, drop_last=False):
    """Multipoles and the 29 tables of a TNS theory at the parameters ``p`` (as tests/test_gpu_tns.py::_oracle_flat); ``drop_last``: the last table wavenumber zeroed."""
    template = theory.template
    q, k11 = template.k, oc.tns_k11(theory.k)
    if not hasattr(theory, '_oracle_kernels'): theory._oracle_kernels = oc.tns_kernels(k11, q, oc.weights_trapz(q))
    pk_q = template.pk_dd_fid * oc.shapefit_factor(q, template.kp, template.a, dm=p.get('dm', 0.), dn=p.get('dn', 0.))
    tables = oc.tns_table_matrix(oc.tns_pt(k11, q, oc.weights_trapz(q), pk_q, kernels=theory._oracle_kernels))
    used = tables.copy()
    if drop_last: used[:, -1] = 0.
    ns = (theory.tracers + '.') if isinstance(theory.tracers, str) else ''
    pt = oc.tns_pktable(theory.k, theory.mu, theory.wmu, q, pk_q, template.f_fid * p.get('df', 1.), qpar=p.get('qpar', 1.), qper=p.get('qper', 1.), sigmav=p.get('sigmav', 0.),
                        fog=theory.fog, kernels=theory._oracle_kernels, k11=k11, tab=used)
    power = oc.tns_tracer_power(pt, theory.nd, b1=p[ns + 'b1'], b2=p.get(ns + 'b2', 0.), bs=p.get(ns + 'bs', 0.), b3=p.get(ns + 'b3', 0.), sn0=p.get(ns + 'sn0', 0.))
    if theory.counterterm_params or theory.stochastic_params:
        power = oc.eftlike_addon(power, list(theory.ells), pt['pk11'], theory.counterterm_matrix, [2. * p.get(n, 0.) for n in theory.counterterm_params], theory.stochastic_matrix,
                                 [p.get(n, 0.) for n in theory.stochastic_params], theory.nd)
    return power, tables


def _kaiser_point(theory, p):
    template = theory.template
    q = template.k
    ns = (theory.tracers + '.') if isinstance(theory.tracers, str) else ''
    pk_q = template.pk_dd_fid * oc.shapefit_factor(q, template.kp, template.a, dm=p.get('dm', 0.), dn=p.get('dn', 0.))
    dd, dt, tt = oc.kaiser_pktable(theory.k, theory.mu, theory.wmu, q, pk_q, template.f_fid * p.get('df', 1.), qpar=p.get('qpar', 1.), qper=p.get('qper', 1.),
                                   sigmapar=p.get('sigmapar', 0.), sigmaper=p.get('sigmaper', 0.))
    return oc.kaiser_tracer_power(theory.ells, dd, dt, tt, theory.nd, p[ns + 'b1'], p[ns + 'b1'], p.get(ns + 'sn0', 0.))


def _bao_point(theory, p):
    """Wiggle multipoles [n_ell, n_kin] of a BAO theory (as tests/test_oracle_bao.py, tests/phaseshift_oracle.py drive the oracle) and its broadband terms (flat, on the theory's
    own output grid)."""
    template = theory.template
    kt, pknow = template.k, template.pknow_dd_fid
    pk_dd = template.pk_dd_fid
    if getattr(template, '_kind', 0) == 4:      # the phase-shift template moves the wiggles (power_template.py:489-492)
        import phaseshift_oracle as pso
        c = dict(ps_k=template.k_wiggles, ps_klim=np.array([template.k_wiggles[0], template.k_wiggles[-1]]), k_t=kt, ps_kshift=template.kshift, ps_wiggles=template.wiggles_fid, pknow_dd_fid=pknow)
        pk_dd = pso.pk_dd(c, p.get('baoshift', 1.))
    f = p.get('dbeta', 1.) * template.f_fid * p.get('df', 1.)
    common = dict(qpar=p.get('qpar', 1.), qper=p.get('qper', 1.), b1=p['b1'], mode=theory.mode, smoothing_radius=theory.smoothing_radius, model=theory.model)
    args = (theory.kin, theory.mu, theory.wmu)
    if theory._flexible:
        matrix = np.zeros((len(theory.ells), len(theory.kin), len(theory.wiggles_params)))
        for iml, ill in enumerate(theory.wiggles_ells): matrix[ill, :, iml] = theory.wiggles_matrix[iml]
        power = oc.bao_flexible_power(*args, theory.ells, kt, pk_dd, pknow, f, matrix, np.array([p.get(n, 0.) for n in theory.wiggles_params]), **common)
    elif theory._resummed:
        scales = oc.bao_resummation_scales(kt, pknow, template.fiducial.rs_drag, mode=theory.mode, smoothing_radius=theory.smoothing_radius)
        power = oc.bao_resummed_power(*args, kt, pk_dd, pknow, f, scales, shotnoise=theory.shotnoise, sigmas=p.get('sigmas', 0.), d=p.get('d', 1.), **common)
    else:
        power = oc.bao_damped_power(*args, kt, pk_dd, pknow, f, sigmas=p.get('sigmas', 0.), sigmapar=p.get('sigmapar', 9.), sigmaper=p.get('sigmaper', 6.), **common)
    broadband = theory.broadband_matrix.dot(np.array([p.get(n, 0.) for n in theory._broadband_names]))
    return power, broadband


def _png_point(theory, p):
    """As tests/test_gpu_png.py::test_host_mirror_matches_oracle; the tracer-velocity variant as tests/test_png_velocity.py."""
    template = theory.template
    kt, fid = template.k, template.fiducial
    pk_dd = template.pk_dd_fid * oc.shapefit_factor(kt, template.kp, template.a, dm=p.get('dm', 0.), dn=p.get('dn', 0.))
    alpha = oc.png_alpha_prim(kt, pk_dd, fid.pk_prim(kt), fid.h)
    bf = oc.png_bfnl(theory.mode, p['b1'], fnl_loc=p.get('fnl_loc', 0.), p=p.get('p', 1.), bphi=p.get('bphi', 1.))
    f = template.f_fid * p.get('df', 1.)
    ap = dict(qpar=p.get('qpar', 1.), qper=p.get('qper', 1.))
    if 'Velocity' in type(theory).__name__:
        return oc.png_velocity_power(theory.k, theory.mu, theory.wmu, kt, pk_dd, alpha, f, theory.z, p['b1'], bf, bv=p.get('bv', 1.), sigmas=p.get('sigmas', 0.), sigmau=p.get('sigmau', 0.), **ap)
    return oc.png_tracer_power(theory.k, theory.mu, theory.wmu, kt, pk_dd, alpha, f, theory.nd, p['b1'], p['b1'], bf, bf, sn0=p.get('sn0', 0.), sigmasX=p.get('sigmas', 0.),
                               sigmasY=p.get('sigmas', 0.), **ap)


def oracle_rows(like, info, theta, drop_last=False):
    """``(loglikelihood [N], theory vector [N, n], tables [N, 29, n11] or None)`` of the rows ``theta`` (columns as ``like.varied_params``; the other parameters at their values).
    ``drop_last``: the contribution of the last table wavenumber (TNS) or of the last ``kin`` column (BAO, PNG) of the first observable is left out -- what a kernel that drops
    its ragged tail would compute (the sensitivity check of tests/test_theory_shapes_cases.py)."""
    varied = like.varied_params.names()
    fixed = {param.name: float(param.value) for param in like.all_params if param.name not in varied}
    family = info['family']
    loglike, flats, tables = [], [], []
    for row in np.atleast_2d(theta):
        p = dict(fixed, **dict(zip(varied, row)))
        flat = []
        for iobs, obs in enumerate(like.observables):
            theory, drop = obs.wmatrix.theory, drop_last and iobs == 0
            xi = hasattr(theory, 's')
            if iobs > 0:
                flat.append(_window(obs, _kaiser_point(theory, p)))
            elif family == 'tns':
                power, tab = _tns_point(theory, p, drop_last=drop)
                tables.append(tab)
                flat.append(_corr(theory, power) if xi else _window(obs, power))
            elif family == 'bao':
                power, broadband = _bao_point(theory, p)
                if xi: flat.append(_corr(theory, power, drop_last=drop) + broadband)
                else: flat.append(_window(obs, power + broadband.reshape(power.shape), drop_last=drop))
            else:
                flat.append(_window(obs, _png_point(theory, p), drop_last=drop))
        flat = np.concatenate(flat)
        flats.append(flat)
        loglike.append(oc.gaussian_loglikelihood(flat, like.flatdata, like.precision)[0])
    return np.array(loglike), np.array(flats), (np.array(tables) if tables else None)


def oracle_power(like, info, theta):
    """Multipoles ``[N, n_ell, n_kin]`` of the first observable in front of its window (what ``Context.eval_theory_host`` returns; BAO: the wiggle multipoles without
    the broadband terms)."""
    varied = like.varied_params.names()
    fixed = {param.name: float(param.value) for param in like.all_params if param.name not in varied}
    theory = like.observables[0].wmatrix.theory
    point = {'tns': lambda p: _tns_point(theory, p)[0], 'bao': lambda p: _bao_point(theory, p)[0], 'png': lambda p: _png_point(theory, p)}[info['family']]
    return np.array([point(dict(fixed, **dict(zip(varied, row)))) for row in np.atleast_2d(theta)])


def oracle_logprior(like, theta):
    return oc.logprior(np.atleast_2d(theta), _priors(like))


def sample(like, size, seed):
    """``theta [size, n_varied]`` drawn as tests/test_gpu_tns.py does: the start distribution where it is proper, the default value otherwise, ``sigmav`` uniform over
    (0.5, 4); clipped into the prior limits."""
    rng = np.random.RandomState(seed)
    params = list(like.varied_params)
    theta = np.column_stack([param.ref.sample(size=size, random_state=rng) if param.ref.is_proper() else np.full(size, param.value) for param in params])
    for i, param in enumerate(params):
        if param.basename == 'sigmav': theta[:, i] = rng.uniform(0.5, 4., size)
        theta[:, i] = np.clip(theta[:, i], *param.prior.limits)
    return theta


def spread_rows(size, count=12):
    """``count`` rows spread over a batch, the last three of the batch always among them."""
    if size <= count: return np.arange(size)
    ntail = min(3, count)
    tail = list(range(size - ntail, size))
    return np.array(sorted(set(tail) | set(np.linspace(0, size - ntail - 1, count - ntail).astype(int).tolist())))
