"""Sample the posterior of the same likelihood given each of N mocks on one MI355X, all mocks at once (cf. the reference: one pipeline and one sampler per mock):

    python examples/sample_mocks.py [number of mocks]

The likelihood of examples/fit_mocks.py: ShapeFit template -> Kaiser tracer multipoles -> windowed P_ell observable -> Gaussian likelihood with the shot-noise term
marginalised analytically; the mocks are the theory at the truth plus noise of the covariance.  ``likelihood.data_batch(mocks)`` holds the mocks on the GPU and
``MockEmceeSampler`` runs two ensembles per mock, every ensemble resident on the device and all of them advancing in lockstep: a half-step of all ensembles is one
small kernel and one batched evaluation, whatever the number of mocks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from desilike_amd import MockEmceeSampler   # noqa: E402
from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles   # noqa: E402
from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, ObservablesCovarianceMatrix, BoxFootprint   # noqa: E402
from desilike_amd.likelihoods import ObservablesGaussianLikelihood   # noqa: E402


def main(nmocks=16, niterations=400, seed=7):
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

    batch = likelihood.data_batch(mocks)                    # sn0 marginalised once: one data vector per mock on the GPU
    sampler = MockEmceeSampler(batch, chains=2, seed=1)     # 2 ensembles per mock, nmocks * 2 ensembles in lockstep
    sampler.run(niterations)
    burnin = niterations // 2
    names = likelihood.varied_params.names()
    mean = np.array([[sampler.to_samples(i, burnin=burnin)[name].mean() for name in names] for i in range(nmocks)])
    std = np.array([[sampler.to_samples(i, burnin=burnin)[name].std(ddof=1) for name in names] for i in range(nmocks)])
    for ip, name in enumerate(names):
        print('  {:6s}: mean of the posterior means {:8.4f}, their scatter {:.4f}, mean posterior error {:.4f}   (truth {:.4f})'.format(name, mean[:, ip].mean(), mean[:, ip].std(ddof=1), std[:, ip].mean(), truth[name]))
    gr = sampler.gelman_rubin(burnin=burnin)
    print('  {:d} ensembles of {:d} walkers, {:d} updates: mean acceptance {:.2f}, max Gelman-Rubin - 1 over the mocks {:.3f}'.format(sampler.n_ensembles, sampler.nwalkers, niterations,
                                                                                                                          sampler.acceptance_fraction.mean(), gr.max()))
    return {'names': names, 'mean': mean, 'std': std, 'truth': truth, 'gelman_rubin': gr, 'sampler': sampler}


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16)
