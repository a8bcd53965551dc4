"""NumPy / scipy oracle of the wiggle-split template (reference: desilike/theories/galaxy_clustering/power_template.py:1150-1214 with integrate_sigma_r2, 1038-1076),
test infrastructure.

Written from the reference's formulas, step by step and without the algebra of the device code (csrc/dl_wigglesplit.h); it works from the flat ``dl_config`` keys
(include/desilike_amd.h) of one observable:

* power_template.py:1193-1194  the inner grid                                                              -> key ``ws_k`` [n_i]
* power_template.py:1196       ``pknow_tt = pknow_tt_interpolator_fid(k)``                                 -> key ``ws_pknow`` [n_i]
* power_template.py:1197       ``wiggles = pk_tt_interpolator_fid(k / qbao) - pknow_tt_interpolator_fid(k / qbao)``: the interpolators are cubic splines in
                               (log10 k, log10 P) of the tables                                            -> keys ``ws_kfid``, ``ws_pk_tt_fid``, ``ws_pknow_tt_fid`` [n_f]
* power_template.py:1199       ``PowerSpectrumInterpolator1D(k, (pknow_tt + wiggles) * (k / kp)**dm)``: the same kind of spline, built per point
* power_template.py:1200       ``norm = df**2 * fsigmar_fid**2 / integrate_sigma_r2(r, interpolator, kernel)``     -> keys ``ws_r``, ``ws_kernel``, ``ws_fsigmar_fid``
* power_template.py:1201-1202  ``pk_dd = interpolator(self.k) * norm / (f_fid * df)**2``

and hands ``pk_dd``, ``f`` to the Kaiser theories of ``oracle/np_oracle.py``.  Window and likelihood follow dl_host.hpp::dl_build_window (tests/phaseshift_oracle.py).
"""
import numpy as np
from scipy import interpolate

from oracle import np_oracle as orc
from phaseshift_oracle import observable_keys, _input, _ap, window, flatdata, precision   # noqa: F401


def _loglog(k, pk):
    spline = interpolate.CubicSpline(np.log10(k), np.log10(pk), bc_type='not-a-knot')
    return lambda kk: 10.**spline(np.log10(kk))


def kernel2(kernel, x):
    """W^2 (power_template.py:973-1030): 0 Gaussian, 1 top-hat with its series below 0.1."""
    if kernel == 0: return np.exp(-x**2)
    toret = np.empty_like(x)
    mask = x < 0.1
    x2 = x[mask]**2
    toret[mask] = (1. + x2 * (-1.0 / 10.0 + x2 * (1.0 / 280.0 + x2 * (-1.0 / 15120.0 + x2 * (1.0 / 1330560.0 + x2 * (-1.0 / 172972800.0))))))**2
    toret[~mask] = (3. * (np.sin(x[~mask]) - x[~mask] * np.cos(x[~mask])) / x[~mask]**3)**2
    return toret


def sigma_r2(r, pk, kernel, kmin=1e-6, kmax=1e2, nk=2048):
    """power_template.py:1071-1076, as written: nodes exp(linspace(log10 kmin, log10 kmax, nk)), trapezoid in that variable."""
    logk = np.linspace(np.log10(kmin), np.log10(kmax), nk)
    k = np.exp(logk)
    integrand = pk(k) * kernel2(kernel, k * r) * k**3
    return 1. / 2. / np.pi**2 * np.sum((integrand[1:] + integrand[:-1]) / 2. * np.diff(logk))


def pk_dd(c, qbao, dm, df=1.):
    """The template's P_dd at its knots ``k_t`` (power_template.py:1192-1202)."""
    k, kp = c['ws_k'], float(c['ws_kp'][0])
    pk_tt_fid, pknow_tt_fid = _loglog(c['ws_kfid'], c['ws_pk_tt_fid']), _loglog(c['ws_kfid'], c['ws_pknow_tt_fid'])
    wiggles = pk_tt_fid(k / qbao) - pknow_tt_fid(k / qbao)
    pk_tt = _loglog(k, (c['ws_pknow'] + wiggles) * (k / kp)**dm)
    norm = df**2 * float(c['ws_fsigmar_fid'][0])**2 / sigma_r2(float(c['ws_r'][0]), pk_tt, int(c['ws_kernel'][0]))
    f = float(c['f_fid'][0]) * df
    return pk_tt(c['k_t']) * norm / f**2


def theory(c, row):
    """(template P_dd [n_t], P_ell(k_in) [n_ell, n_kin]) of one observable at the parameter row ``row``."""
    qpar, qper = _ap(c, row)
    df = _input(c, 'df', row, 1.)
    f = float(c['f_fid'][0]) * df
    pk11 = pk_dd(c, _input(c, 'qbao', row, 1.), _input(c, 'dm', row, 0.), df=df)
    nell, nkin = len(c['ells_in']), len(c['kin'])
    ells = tuple(int(ell) for ell in c['ells_in'])
    dd, dt, tt = orc.kaiser_pktable(c['kin'], c['mu'], c['wmu_ell'].reshape(nell, -1), c['k_t'], pk11, f, qpar=qpar, qper=qper,
                                    sigmapar=_input(c, 'sigmapar', row, 0.), sigmaper=_input(c, 'sigmaper', row, 0.))
    nd = float(c['nd'][0])
    power = orc.kaiser_tracer_power(ells, dd, dt, tt, nd, _input(c, 'b1X', row, 1.), _input(c, 'b1Y', row, 1.), _input(c, 'sn0', row, 0.))
    if 'ct_matrix' in c or 'sn_matrix' in c:
        value = lambda pair: row[int(round(pair[0]))] if pair[0] >= 0 else pair[1]   # noqa: E731
        ctm = c['ct_matrix'].reshape(nell, nkin, -1) if 'ct_matrix' in c else np.zeros((nell, nkin, 0))
        snm = c['sn_matrix'].reshape(nell, nkin, -1) if 'sn_matrix' in c else np.zeros((nell, nkin, 0))
        ct = [value(pairs[0]) + value(pairs[1]) for pairs in c['in.ct'].reshape(-1, 2, 2)] if ctm.size else []
        sn = [value(pair) for pair in c['in.sn'].reshape(-1, 2)] if snm.size else []
        power = orc.eftlike_addon(power, ells, dd, ctm, ct, snm, sn, nd)
    return pk11, power


def flattheory(cfg, row):
    """Theory vector of all observables, the list of their multipoles and of their templates."""
    flat, powers, templates = [], [], []
    for iobs in range(int(cfg['n_obs'][0])):
        c = observable_keys(cfg, iobs)
        pk11, power = theory(c, row)
        W, bias = window(c)
        flat.append(W.dot(np.ravel(power)) + bias)
        powers.append(power); templates.append(pk11)
    return np.concatenate(flat), powers, templates


def loglikelihood(cfg, row):
    return orc.gaussian_loglikelihood(flattheory(cfg, row)[0], flatdata(cfg), precision(cfg))[0]
