"""Fixtures of the BAO phase-shift template, from the REFERENCE side (build container only; the reference never travels to the GPU box):

    python tests/golden/make_phaseshift_fixture.py [name ...]

Builds real desilike likelihoods on the reference's own ``BAOPhaseShiftPowerSpectrumTemplate`` (power_template.py:442-496; through tests/golden/refstub for the absent
cosmoprimo / lsstypes), runs ``integration/desilike_mi355x.py::extract_config`` on them and stores in ``boundary_phaseshift_<name>.npz`` the flat ``dl_config`` key ->
array set (``cfg/<key>``), 48 points (``baoshift`` uniform over its prior, rows 0, 1, 2 at exactly -8, 1, 10) with the parameter names and prior limits, and the
reference's own numbers at them: ``wiggle_power`` (the wiggle multipoles P_ell(k_in) of every observable, concatenated), ``flattheory``, ``loglikelihood``,
``logprior``, ``logposterior``; ``params/*``: what the reference's parameter file gives the template (power_template.yaml:174-216).

The reference reads the ends of its inner wiggle grid off the cosmoprimo interpolator (``extrap_kmin`` / ``extrap_kmax``, power_template.py:490); the stub's ``SyntheticPk``
has no such attributes: they are set on the class HERE, the stub stays as it is.  The archives are written with fixed time stamps: regenerating gives the same bytes.
"""
import io
import os
import sys
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

from cosmoprimo.cosmology import SyntheticPk

from desilike.theories.galaxy_clustering import (BAOPhaseShiftPowerSpectrumTemplate, DampedBAOWigglesTracerPowerSpectrumMultipoles, DampedBAOWigglesTracerCorrelationFunctionMultipoles,
                                                 ResummedBAOWigglesTracerPowerSpectrumMultipoles, FlexibleBAOWigglesTracerPowerSpectrumMultipoles)
from desilike.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, TracerCorrelationFunctionMultipolesObservable
from desilike.likelihoods import ObservablesGaussianLikelihood
from desilike.base import vmap

from desilike_mi355x import extract_config
from make_golden import sample_theta

SELECTED = set(sys.argv[1:])     # fixture names to (re)generate; none: all of them
SIZE = 48


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


def dump(name, build, klim=(1e-5, 1e2), seed=42):
    if SELECTED and name not in SELECTED: return
    SyntheticPk.extrap_kmin, SyntheticPk.extrap_kmax = klim
    likelihood = build()
    likelihood()
    cfg = extract_config(likelihood)
    names = [str(n) for n in cfg['__varied__']]
    theta = sample_theta(likelihood, SIZE, seed)
    ishift = names.index('baoshift')
    theta[:3, ishift] = [-8., 1., 10.]
    out = {'cfg/' + key: value for key, value in cfg.items() if not key.startswith('__')}
    limits = np.array([likelihood.varied_params[n].prior.limits for n in names], dtype='f8')
    (logpost, derived), errors = vmap(likelihood, backend=None, errors='return', return_derived=True)({n: theta[:, i] for i, n in enumerate(names)})
    assert not errors, errors
    power, flat = [], []
    for row in theta:
        likelihood(**dict(zip(names, row)))
        wiggle = []
        for obs in likelihood.observables:
            theory = obs.wmatrix.theory
            pt = theory.power if hasattr(theory, 'get_corr') else theory.pt
            wiggle.append(np.ravel(np.asarray(pt.power, dtype='f8')))
        power.append(np.concatenate(wiggle))
        flat.append(np.asarray(likelihood.flattheory, dtype='f8').copy())
    out.update(names=np.array(names), theta=theta, prior_limits=limits, wiggle_power=np.array(power), flattheory=np.array(flat),
               loglikelihood=np.asarray(derived[likelihood._param_loglikelihood]), logprior=np.asarray(derived[likelihood._param_logprior]), logposterior=np.asarray(logpost))
    # the template's parameters as the reference's parameter file gives them, in its order
    template = likelihood.observables[0].wmatrix.theory
    template = (template.power if hasattr(template, 'get_corr') else template.pt).template
    tparams = list(template.init.params)
    out['params/names'] = np.array([param.basename for param in tparams])
    out['params/value'] = np.array([param.value for param in tparams], dtype='f8')
    out['params/prior_limits'] = np.array([param.prior.limits for param in tparams], dtype='f8')
    out['params/ref_limits'] = np.array([param.ref.limits for param in tparams], dtype='f8')
    out['params/delta'] = np.array([np.nan if param._delta is None else np.ravel(param._delta)[0] for param in tparams], dtype='f8')   # (first entry: the step; nan: none given)
    out['params/fixed'] = np.array([bool(param.fixed) for param in tparams])
    out['params/latex'] = np.array([str(param.latex()) for param in tparams])
    fn = os.path.join(here, 'boundary_phaseshift_{}.npz'.format(name))
    savez_reproducible(fn, out)
    shifted = cfg['obs0.k_t'][None, :] + (theta[:, ishift, None] - 1.) * cfg['obs0.ps_kshift'][None, :]
    print('saved', fn, '{:.1f} kB'.format(os.path.getsize(fn) / 1e3), 'keys', len(cfg) - 2, 'knots clipped below / above:', int((shifted < klim[0]).sum()), int((shifted > klim[1]).sum()))


def pk_observable(theory, nk=56, shotnoise=None, **data):
    return TracerPowerSpectrumMultipolesObservable(data=data, kedges=np.linspace(0.02, 0.3, nk + 1), ells=(0, 2), wmatrix={'resolution': 3}, theory=theory, shotnoise=shotnoise)


def free_damping(theory):
    for name in ['sigmapar', 'sigmaper']: theory.init.params[name].update(fixed=False, ref=dict(dist='norm', loc=8., scale=0.5))


def damped_pk(apmode='qparqper'):
    theory = DampedBAOWigglesTracerPowerSpectrumMultipoles(template=BAOPhaseShiftPowerSpectrumTemplate(z=0.5, apmode=apmode), model='standard')
    free_damping(theory)
    return ObservablesGaussianLikelihood(observables=[pk_observable(theory, b1=2., sigmas=2.)], covariance=covariance(112, 30.))


def damped_xi():
    theory = DampedBAOWigglesTracerCorrelationFunctionMultipoles(template=BAOPhaseShiftPowerSpectrumTemplate(z=0.5), mode='reciso')
    free_damping(theory)
    obs = TracerCorrelationFunctionMultipolesObservable(data={'b1': 2., 'sigmas': 2.}, s=np.linspace(22.5, 167.5, 30), ells=(0, 2), theory=theory)
    return ObservablesGaussianLikelihood(observables=[obs], covariance=covariance(60, 3e-4))


def models():
    """Phase-B variants 1, 2, 3 of the BAO kernel: the 'fix-damping move-all fog-damping' family, resummed wiggles, flexible wiggles -- one observable each, one shared template."""
    template = BAOPhaseShiftPowerSpectrumTemplate(z=0.5)
    theories = [DampedBAOWigglesTracerPowerSpectrumMultipoles(template=template, mode='recsym', model='fog-damping_move-all'),
                ResummedBAOWigglesTracerPowerSpectrumMultipoles(template=template, mode='reciso', model='standard'),
                FlexibleBAOWigglesTracerPowerSpectrumMultipoles(template=template, mode='reciso', model='standard', wiggles='pcs')]
    free_damping(theories[0])
    theories[1].init.params['d'].update(fixed=False)
    observables = []
    for theory in theories:
        for param in theory.init.params.select(basename='al*'): param.update(fixed=True)
        for param in theory.init.params.select(basename='ml*'): param.update(ref=dict(limits=[-0.3, 0.3]))
        data = {'b1': 2.} if theory is theories[2] else {'b1': 2., 'sigmas': 2.}
        observables.append(pk_observable(theory, nk=28, shotnoise=3e3 if theory is theories[1] else None, **data))   # (28 bins: three observables in one archive below the size limit)
    return ObservablesGaussianLikelihood(observables=observables, covariance=covariance(168, 30.))


def main():
    dump('pk', damped_pk, seed=81)
    dump('xi', damped_xi, seed=83)
    dump('models', models, seed=85)
    dump('clip', lambda: damped_pk(apmode='qiso'), klim=(2e-4, 1.01), seed=87)


if __name__ == '__main__':
    main()
