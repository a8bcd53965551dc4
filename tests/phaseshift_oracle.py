"""NumPy / scipy oracle of the BAO phase-shift template (reference: desilike/theories/galaxy_clustering/power_template.py:442-496, Baumann et al. 2018), test infrastructure.

Written from the reference's formulas, independent of the device code; it works from the flat ``dl_config`` keys (include/desilike_amd.h) of one observable:

* power_template.py:489   ``kshift = phiinf / (1 + (kstar / k)^epsilon) / rs_drag``                                  -> key ``ps_kshift`` [n_t]
* power_template.py:490   ``k = geomspace(extrap_kmin, extrap_kmax, 2000)``                                          -> key ``ps_k`` [n_w], ``ps_klim`` [2]
* power_template.py:491   ``wiggles = _interp(clip(self.k + (baoshift - 1) kshift, k[0], k[-1]), k, pk_fid(k) - pknow_fid(k))`` -> key ``ps_wiggles`` [n_w]
* power_template.py:492   ``pk_dd = pknow_dd_fid + wiggles``
* power_template.py:436-439 ``_interp``: cubic in log10 k; without interpax it is ``scipy.interpolate.interp1d(kind='cubic')``: the not-a-knot spline

and hands ``pk_dd`` to the BAO wiggle theories of ``oracle/np_oracle.py`` (bao.py:117-151, 165-266, 269-391), which spline ``pk_dd`` and ``pknow_dd`` again on the template knots
(bao.py:121-125).  Window, broadband (pass-through) columns and the Gaussian likelihood follow dl_host.hpp::dl_build_window: ``flattheory = W [P_ell, broadband] + bias``.
"""
import numpy as np
from scipy import interpolate

from oracle import np_oracle as orc


def observable_keys(cfg, iobs=0):
    prefix = 'obs{:d}.'.format(iobs)
    return {key[len(prefix):]: np.asarray(value) for key, value in cfg.items() if key.startswith(prefix)}


def shifted_wiggles(c, baoshift):
    """Wiggles at the template knots [n_t] (power_template.py:489-491); the clip comes before the logarithm."""
    kw = c['ps_k']
    klim = c['ps_klim'] if 'ps_klim' in c else (kw[0], kw[-1])
    k = np.clip(c['k_t'] + (baoshift - 1.) * c['ps_kshift'], klim[0], klim[1])
    return interpolate.interp1d(np.log10(kw), c['ps_wiggles'], kind='cubic', fill_value='extrapolate', assume_sorted=True)(np.log10(k))


def pk_dd(c, baoshift):
    """power_template.py:492; without the phase-shift keys (``BAOPowerSpectrumTemplate``): the fiducial spectrum itself."""
    if 'ps_k' not in c: return c['pk_dd_fid']
    return c['pknow_dd_fid'] + shifted_wiggles(c, baoshift)


def _input(c, name, row, default):
    if 'in.' + name not in c: return default
    col, value = c['in.' + name][:2]
    return row[int(round(col))] if col >= 0 else value


def _ap(c, row):
    """theories/galaxy_clustering/base.py:341-350."""
    apmode, eta = int(c['apmode'][0]), float(c['eta'][0])
    if apmode == 0: return _input(c, 'qpar', row, 1.), _input(c, 'qper', row, 1.)
    qiso = _input(c, 'qiso', row, 1.) if apmode in (1, 3) else 1.
    qap = _input(c, 'qap', row, 1.) if apmode in (2, 3) else 1.
    return qiso * qap**(1. - eta), qiso * qap**(-eta)


def wiggle_power(c, row):
    """P_ell(k_in) [n_ell, n_kin] of one observable at the parameter row ``row``."""
    qpar, qper = _ap(c, row)
    bits = int(c['bao_mode'][0])
    mode, model_bits = ('reciso' if bits & 15 else 'recsym'), bits >> 4       # ('' and 'recsym' are the same model: bao.py:131)
    model = 'standard' if not (model_bits & 7) else '_'.join(word for bit, word in [(1, 'fix-damping'), (2, 'move-all'), (4, 'fog-damping')] if model_bits & bit)
    f = _input(c, 'dbeta', row, 1.) * float(c['f_fid'][0]) * _input(c, 'df', row, 1.)            # bao.py:119, power_template.py:374
    common = dict(qpar=qpar, qper=qper, b1=_input(c, 'b1X', row, 1.), mode=mode, smoothing_radius=float(c['smoothing_radius'][0]), model=model)
    nell = len(c['ells_in'])
    args = (c['kin'], c['mu'], c['wmu_ell'].reshape(nell, -1), c['k_t'], pk_dd(c, _input(c, 'baoshift', row, 1.)), c['pknow_dd_fid'], f)
    if model_bits & 32:
        nml = len(c['ml_ell'])
        values = np.array([row[int(round(col))] if col >= 0 else value for col, value in c['in.ml'].reshape(nml, 2)])
        matrix = np.zeros((nell, len(c['kin']), nml))
        for q, ill in enumerate(c['ml_ell']): matrix[ill, :, q] = c['ml_matrix'].reshape(nml, -1)[q]
        return orc.bao_flexible_power(args[0], args[1], args[2], tuple(int(ell) for ell in c['ells_in']), *args[3:], matrix, values, **common)
    if model_bits & 16:
        sdd2, snl2, sx2, sn = c['resummed']
        return orc.bao_resummed_power(*args, (sdd2, snl2, sx2, sn), shotnoise=1., sigmas=_input(c, 'sigmas', row, 0.), d=_input(c, 'dres', row, 1.), **common)
    return orc.bao_damped_power(*args, sigmas=_input(c, 'sigmas', row, 0.), sigmapar=_input(c, 'sigmapar', row, 9.), sigmaper=_input(c, 'sigmaper', row, 6.), **common)


def window(c):
    """(W [n_out, n_in + n_pass], bias [n_out]) as dl_host.hpp::dl_build_window folds them."""
    nell, nkin = len(c['ells_in']), len(c['kin'])
    npass = c['in.pass'].size // 2 if 'in.pass' in c else 0
    W = c['wmatrix'].reshape(-1, nell * nkin + npass)
    bias = np.zeros(W.shape[0])
    if 'shotnoise_in' in c: bias += sum(W[:, ill * nkin:(ill + 1) * nkin].sum(axis=1) * sn for ill, sn in enumerate(c['shotnoise_in']))
    if 'offset' in c: bias += c['offset']
    if 'shotnoise_out' in c: bias -= c['shotnoise_out']
    return W, bias


def flattheory(cfg, row, power=None):
    """Theory vector of all observables (and the list of their wiggle multipoles); ``power``: precomputed wiggle multipoles per observable."""
    flat, powers = [], []
    for iobs in range(int(cfg['n_obs'][0])):
        c = observable_keys(cfg, iobs)
        p = wiggle_power(c, row) if power is None else power[iobs]
        W, bias = window(c)
        npass = W.shape[1] - p.size
        passed = np.array([row[int(round(col))] if col >= 0 else value for col, value in c['in.pass'].reshape(npass, 2)]) if npass else np.zeros(0)
        flat.append(W.dot(np.concatenate([np.ravel(p), passed])) + bias)
        powers.append(p)
    return np.concatenate(flat), powers


def flatdata(cfg):
    return np.concatenate([observable_keys(cfg, iobs)['flatdata'] for iobs in range(int(cfg['n_obs'][0]))])


def precision(cfg):
    n = flatdata(cfg).size
    matrix = np.asarray(cfg['precision'])
    return matrix.reshape(n, n) if matrix.size == n * n else np.diag(matrix)


def loglikelihood(cfg, row):
    return orc.gaussian_loglikelihood(flattheory(cfg, row)[0], flatdata(cfg), precision(cfg))[0]
