"""Sample the posterior of the same likelihood given each of N mocks with the nuisance term marginalised analytically, then draw the marginalised parameter at every
chain point, all mocks at once on one MI355X:

    python examples/sample_mocks_solved.py [number of mocks]

The likelihood of examples/sample_mocks.py (ShapeFit template -> Kaiser tracer multipoles -> windowed P_ell observable -> Gaussian likelihood, the shot-noise term sn0
'.marg').  ``likelihood.data_batch(mocks, solve='point')`` solves sn0 per point and per mock, ``MockEmceeSampler`` samples the other parameters of every mock, and
``sampler.sample_solved`` draws sn0 from its conditional Gaussian at every chain point, each chain against its own mock -- a few chunked calls for all mocks together.  The
chains it returns hold all parameters, with ``loglikelihood + logprior = logposterior`` un-marginalised."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from desilike_amd import MockEmceeSampler   # noqa: E402
from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles   # noqa: E402
from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable, ObservablesCovarianceMatrix, BoxFootprint   # noqa: E402
from desilike_amd.likelihoods import ObservablesGaussianLikelihood   # noqa: E402


def main(nmocks=4, niterations=120, size=2, seed=7):
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

    batch = likelihood.data_batch(mocks, solve='point')     # sn0 solved per point and per mock
    sampler = MockEmceeSampler(batch, chains=2, seed=1)     # 2 ensembles per mock, sampling the other parameters
    sampler.run(niterations)
    burnin = niterations // 2
    chains = sampler.sample_solved(size=size, seed=3, burnin=burnin)      # chains[i][k]: every column repeated `size` times, sn0 drawn, nothing marginalised
    sampled, solved = likelihood.varied_params.names(), likelihood.solved_params.names()
    mean = np.array([[np.mean([chain[name] for chain in chains[i]]) for name in sampled + solved] for i in range(nmocks)])
    print('  per-mock posterior means ({:d} updates after burn-in, {:d} draws of the solved parameters per point)'.format(niterations - burnin, size))
    print('  mock ' + ' '.join('{:>9s}'.format(name) for name in sampled + solved))
    for i in range(nmocks):
        print('  {:4d} '.format(i) + ' '.join('{:9.4f}'.format(value) for value in mean[i]))
    print(' truth ' + ' '.join('{:9.4f}'.format(truth[name]) for name in sampled + solved))
    identity = max(np.abs(chain['loglikelihood'] + chain['logprior'] - chain['logposterior']).max() for row in chains for chain in row)
    print('  max |loglikelihood + logprior - logposterior| over the chains: {:.1e}'.format(identity))
    return {'names': sampled + solved, 'mean': mean, 'truth': truth, 'chains': chains, 'sampler': sampler}


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4)
