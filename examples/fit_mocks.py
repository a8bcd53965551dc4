"""Fit the same likelihood to each of N mocks on one MI355X, as ONE batch (cf. the reference: one pipeline per mock, farmed over MPI):

    python examples/fit_mocks.py [number of mocks]

ShapeFit template -> Kaiser tracer multipoles -> windowed P_ell observable -> Gaussian likelihood with the shot-noise term marginalised analytically.  The mocks are
the theory at the truth plus noise of the covariance.  ``GaussNewtonProfiler.maximize_batch`` maximises the posterior of every mock as rows of one Levenberg-Marquardt
batch (the Gauss-Newton curvature does not depend on the data: one theory evaluation and one window product per row whatever the mock); ``likelihood.data_batch``
then gives the log-posterior of any point against every mock in one call -- here the best fit of every mock against every mock."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles   # noqa: E402
from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, ObservablesCovarianceMatrix, BoxFootprint   # noqa: E402
from desilike_amd.likelihoods import ObservablesGaussianLikelihood   # noqa: E402
from desilike_amd.profilers import GaussNewtonProfiler   # noqa: E402


def main(nmocks=25, seed=7):
    template = ShapeFitPowerSpectrumTemplate(z=0.8, fiducial='synthetic', apmode='qiso')
    nbar = 2e-2
    theory = KaiserTracerPowerSpectrumMultipoles(template=template, shotnoise=1. / nbar)
    truth = {'b1': 1.8, 'qiso': 1.01, 'dm': 0.01, 'df': 0.98, 'sn0': 0.1}
    observable = TracerPowerSpectrumMultipolesObservable(data=truth, kedges=np.linspace(0.01, 0.2, 39), ells=(0, 2, 4), wmatrix={'resolution': 5}, theory=theory, shotnoise=1. / nbar)
    covariance = ObservablesCovarianceMatrix(observable, footprints=BoxFootprint(volume=2e10, nbar=nbar), resolution=3)(**truth)
    likelihood = ObservablesGaussianLikelihood(observables=[observable], covariance=covariance)
    likelihood.all_params = {'sn0': {'derived': '.marg'}}
    likelihood.initialize()
    mocks = np.random.RandomState(seed).multivariate_normal(likelihood.flatdata, covariance, size=nmocks)      # [nmocks, n_data], the order of likelihood.flatdata

    profiler = GaussNewtonProfiler(likelihood, seed=1)
    names = [param.name for param in profiler.params]
    profiles = profiler.maximize_batch(mocks, nstarts=2)                       # a list of nmocks Profiles
    best = np.array([[profile.choice()[name] for name in names] for profile in profiles])
    error = np.array([[profile.error[name][profile.argmax()] for name in names] for profile in profiles])
    for ip, name in enumerate(names):
        print('  {:6s}: mean of the best fits {:8.4f}, their scatter {:.4f}, mean error {:.4f}   (truth {:.4f})'.format(name, best[:, ip].mean(), best[:, ip].std(ddof=1), error[:, ip].mean(), truth[name]))

    batch = likelihood.data_batch(mocks)                                       # sn0 marginalised: the marginalised-precision context, one data vector per mock
    varied = likelihood.varied_params.names()
    table = batch.logposterior(best[:, [names.index(name) for name in varied]])   # [nmocks, nmocks]: best fit of mock b given mock m
    print('  the best fit of every mock has the highest log-posterior given that mock:', bool((np.diag(table)[None, :] >= table - 1e-6).all()))
    return {'names': names, 'best': best, 'error': error, 'truth': truth, 'table': table}


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 25)
