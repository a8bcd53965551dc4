"""Fixtures of the wiggle-split template, from the REFERENCE side (build container only; the reference never travels to the GPU box):

    python tests/golden/make_wigglesplit_fixture.py [name ...]

Builds real desilike likelihoods on the reference's own ``WiggleSplitPowerSpectrumTemplate`` (power_template.py:1150-1214; through tests/golden/refstub for the absent
cosmoprimo / lsstypes), runs ``integration/desilike_mi355x.py::extract_config`` on them and stores in ``boundary_wigglesplit_<name>.npz`` the flat ``dl_config`` key ->
array set (``cfg/<key>``), 48 points with the parameter names and prior limits, and the reference's own numbers at them: the template's ``pk_dd`` at its knots and ``f``,
``theory_obs<i>`` (the multipoles P_ell(k_in) of every observable), ``flattheory``, ``loglikelihood``, ``logprior``, ``logposterior``; ``params/*``: what the
reference's parameter file gives the template (power_template.yaml:351-388); ``ref_seconds_per_eval``: the reference's time per likelihood call HERE, through the stub.
Rows 0-5 sit exactly on qbao = 0.8 / 1.2, dm = -3 / 3, df = 0.5 / 1.5; qbao, qap and dm of the others are uniform over their priors, df over [0.5, 1.5].

The template evaluates cosmoprimo interpolators at arbitrary wavenumbers: the stub's analytic ``SyntheticPk`` is replaced HERE (the stub stays as it is) by a TABULATED
interpolator, the project's own ``desilike_amd.fiducial.LogLogSpline`` (not-a-knot cubic spline in (log10 k, log10 P)) of ``SyntheticPk`` on ``geomspace(*klim, 1400)``,
with ``to_1d``, ``clone(wiggle=0.)`` (the no-wiggle table) and ``extrap_kmin`` / ``extrap_kmax``; ``power_template.PowerSpectrumInterpolator1D`` is replaced by the same
spline.  The fixtures therefore pin everything the reference does downstream of the interpolator, not cosmoprimo's interpolator itself.  The archives are written with
fixed time stamps: regenerating gives the same bytes (but for ``ref_seconds_per_eval``).
"""
import io
import os
import sys
import time
import warnings
import zipfile

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
sys.path.insert(0, os.path.join(here, 'refstub'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'integration'))
warnings.filterwarnings('ignore')

from cosmoprimo import cosmology as stub_cosmology
from cosmoprimo.cosmology import SyntheticPk

from desilike.theories.galaxy_clustering import power_template as ref_power_template
from desilike.theories.galaxy_clustering import (WiggleSplitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles, KaiserTracerCorrelationFunctionMultipoles,
                                                 EFTLikeKaiserTracerPowerSpectrumMultipoles)
from desilike.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, TracerCorrelationFunctionMultipolesObservable
from desilike.likelihoods import ObservablesGaussianLikelihood
from desilike.base import vmap

from desilike_amd.fiducial import LogLogSpline
from desilike_mi355x import extract_config
from make_golden import sample_theta

SELECTED = set(sys.argv[1:])     # fixture names to (re)generate; none: all of them
SIZE = 48
NK_TABLE = 1400
KLIM = [1e-5, 1e2]               # ends of the tabulated interpolators (set by dump)


class TabulatedPk(LogLogSpline):
    """The stand-in for a cosmoprimo interpolator: tables of the stub's analytic spectrum with and without wiggles."""

    def __init__(self, k, pk, pknow):
        super(TabulatedPk, self).__init__(k, pk)
        self.pknow = np.array(pknow, dtype='f8')

    def to_1d(self, **kwargs):
        return self

    def clone(self, wiggle=None, **kwargs):
        assert wiggle == 0. and not kwargs
        return TabulatedPk(self.k, self.pknow, self.pknow)


def pk_interpolator(self, of='delta_cb', **kwargs):
    of = of if isinstance(of, str) else of[0]
    analytic = SyntheticPk(scale={'delta_cb': 1., 'theta_cb': 0.64}[of], rs=self.cosmo.rs_drag, n_s=self.cosmo.n_s)
    k = np.geomspace(KLIM[0], KLIM[1], NK_TABLE)
    return TabulatedPk(k, analytic(k), analytic.clone(wiggle=0.)(k))


stub_cosmology._Fourier.pk_interpolator = pk_interpolator
ref_power_template.PowerSpectrumInterpolator1D = lambda k, pk, **kwargs: LogLogSpline(k, pk)


def covariance(n, scale, seed=4):
    rng = np.random.RandomState(seed)
    A = rng.standard_normal((n, n)) * scale
    return A.dot(A.T) + (10. * scale)**2 * np.eye(n)


def savez_reproducible(fn, arrays):
    with zipfile.ZipFile(fn, 'w', compression=zipfile.ZIP_DEFLATED) as archive:
        for key in sorted(arrays):
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buffer.getvalue())


def find_template(likelihood):
    theory = likelihood.observables[0].wmatrix.theory
    return (theory.power if hasattr(theory, 'get_corr') else theory).template


def dump(name, build, klim=(1e-5, 1e2), seed=42):
    if SELECTED and name not in SELECTED: return
    KLIM[:] = klim
    likelihood = build()
    likelihood()
    cfg = extract_config(likelihood)
    # a template shared by several theories takes the knots that cover them all (full_shape.py:29), but the parameter queries of extract_config re-initialise the
    # calculators one after the other: the knots it read for the later observables are not the ones the evaluations below use.  Read them again after an evaluation.
    likelihood()
    for iobs, obs in enumerate(likelihood.observables):
        theory = obs.wmatrix.theory
        template = (theory.power if hasattr(theory, 'get_corr') else theory).template
        cfg['obs{:d}.k_t'.format(iobs)], cfg['obs{:d}.pk_dd_fid'.format(iobs)] = np.asarray(template.k, dtype='f8').copy(), np.asarray(template.pk_dd_fid, dtype='f8').copy()
    names = [str(n) for n in cfg['__varied__']]
    theta = sample_theta(likelihood, SIZE, seed)
    rng = np.random.RandomState(seed + 1)
    spans = {'qbao': (0.8, 1.2), 'qap': (0.8, 1.2), 'dm': (-3., 3.), 'df': (0.5, 1.5)}
    for pname, (lo, hi) in spans.items():
        theta[:, names.index(pname)] = rng.uniform(lo, hi, SIZE)
    corners = [('qbao', 0.8), ('qbao', 1.2), ('dm', -3.), ('dm', 3.), ('df', 0.5), ('df', 1.5)]
    for row, (pname, value) in enumerate(corners): theta[row, names.index(pname)] = value
    out = {'cfg/' + key: value for key, value in cfg.items() if not key.startswith('__')}
    limits = np.array([likelihood.varied_params[n].prior.limits for n in names], dtype='f8')
    (logpost, derived), errors = vmap(likelihood, backend=None, errors='return', return_derived=True)({n: theta[:, i] for i, n in enumerate(names)})
    assert not errors, errors
    pk_dd, f, flat = [], [], []
    theories = [[] for obs in likelihood.observables]
    t0 = time.time()
    for row in theta: likelihood(**dict(zip(names, row)))
    seconds = (time.time() - t0) / len(theta)
    for row in theta:
        likelihood(**dict(zip(names, row)))
        template = find_template(likelihood)
        pk_dd.append(np.asarray(template.pk_dd, dtype='f8').copy()); f.append(float(template.f))
        for iobs, obs in enumerate(likelihood.observables):
            theory = obs.wmatrix.theory
            theories[iobs].append(np.ravel(np.asarray((theory.power if hasattr(theory, 'get_corr') else theory).power, dtype='f8')).copy())
        flat.append(np.asarray(likelihood.flattheory, dtype='f8').copy())
    out.update(names=np.array(names), theta=theta, prior_limits=limits, pk_dd=np.array(pk_dd), f=np.array(f), flattheory=np.array(flat),
               loglikelihood=np.asarray(derived[likelihood._param_loglikelihood]), logprior=np.asarray(derived[likelihood._param_logprior]), logposterior=np.asarray(logpost),
               ref_seconds_per_eval=np.array([seconds]))
    for iobs, rows in enumerate(theories): out['theory_obs{:d}'.format(iobs)] = np.array(rows)
    # the template's parameters as the reference's parameter file gives them, in its order (derived ones -- r -- left out)
    tparams = [param for param in find_template(likelihood).init.params if not param.derived]
    out['params/names'] = np.array([param.basename for param in tparams])
    out['params/value'] = np.array([param.value for param in tparams], dtype='f8')
    out['params/prior_limits'] = np.array([param.prior.limits for param in tparams], dtype='f8')
    out['params/ref_limits'] = np.array([param.ref.limits for param in tparams], dtype='f8')
    out['params/delta'] = np.array([np.nan if param._delta is None else np.ravel(param._delta)[0] for param in tparams], dtype='f8')   # (first entry: the step; nan: none given)
    out['params/fixed'] = np.array([bool(param.fixed) for param in tparams])
    out['params/latex'] = np.array([str(param.latex()) for param in tparams])
    fn = os.path.join(here, 'boundary_wigglesplit_{}.npz'.format(name))
    savez_reproducible(fn, out)
    print('saved', fn, '{:.1f} kB'.format(os.path.getsize(fn) / 1e3), 'keys', len(cfg) - 2, 'inner knots', len(cfg['obs0.ws_k']), 'reference {:.2f} ms per call'.format(1e3 * seconds))


def kaiser():
    theory = KaiserTracerPowerSpectrumMultipoles(template=WiggleSplitPowerSpectrumTemplate(z=0.5))
    obs = TracerPowerSpectrumMultipolesObservable(data={'b1': 2., 'sn0': 0.2}, kedges=np.linspace(0.02, 0.3, 41), ells=(0, 2, 4), wmatrix={'resolution': 3}, theory=theory)
    return ObservablesGaussianLikelihood(observables=[obs], covariance=covariance(120, 30.))


def tophat_eft():
    theory = EFTLikeKaiserTracerPowerSpectrumMultipoles(template=WiggleSplitPowerSpectrumTemplate(z=0.5, kernel='tophat', r=10.))
    obs = TracerPowerSpectrumMultipolesObservable(data={'b1': 1.8, 'ct0_2': 1.5}, kedges=np.linspace(0.02, 0.25, 31), ells=(0, 2, 4), wmatrix={'resolution': 3}, theory=theory, shotnoise=1e4)
    return ObservablesGaussianLikelihood(observables=[obs], covariance=covariance(90, 30.))


def two():
    """Two tracers on ONE template (its evaluation is shared on the device), and the correlation function of the first."""
    template = WiggleSplitPowerSpectrumTemplate(z=0.5)
    observables = []
    for tracer, kmax, b1, shotnoise in [('LRG', 0.2, 2., 1e4), ('ELG', 0.15, 1.3, 4e3)]:
        theory = KaiserTracerPowerSpectrumMultipoles(template=template, tracers=tracer)
        nk = int(round((kmax - 0.02) / 0.01))
        observables.append(TracerPowerSpectrumMultipolesObservable(data={tracer + '.b1': b1}, kedges=np.linspace(0.02, kmax, nk + 1), ells=(0, 2), wmatrix={'resolution': 3},
                                                                   theory=theory, shotnoise=shotnoise))
    theory = KaiserTracerCorrelationFunctionMultipoles(template=template, tracers='LRG')
    observables.append(TracerCorrelationFunctionMultipolesObservable(data={'LRG.b1': 2.}, s=np.linspace(22.5, 147.5, 26), ells=(0, 2), theory=theory))
    n = sum(len(np.ravel(obs.flatdata)) for obs in observables)
    cov = covariance(n, 30.)
    nxi = 52
    cov[-nxi:, :] *= 1e-5; cov[:, -nxi:] *= 1e-5   # (the correlation function's numbers are ~1e-5 of the power spectrum's)
    return ObservablesGaussianLikelihood(observables=observables, covariance=cov)


def main():
    dump('kaiser', kaiser, seed=91)
    dump('tophat_eft', tophat_eft, klim=(1e-4, 30.), seed=93)
    dump('two', two, seed=95)


if __name__ == '__main__':
    main()
