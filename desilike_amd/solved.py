"""Posterior draws of analytically marginalised ("solved") parameters at the points of a chain: ``Chain.sample_solved`` of the reference
(samples/chain.py:229-263, called by its ``to_getdist``), on the GPU (``dl_sample_solved``, csrc/dl_sample_solved.h).

The chains the samplers return hold the sampled parameters only; the '.marg' / '.best' / '.auto' parameters are solved at every point.  :func:`sample_solved`
evaluates the points again, draws the solved parameters from their conditional Gaussian (mean: the solution, precision: minus the Hessian of the log-posterior)
and undoes the marginalisation terms, so that ``loglikelihood + logprior = logposterior`` of the result is the log-posterior with nothing marginalised."""
import warnings

import numpy as np

from .parameter import Samples

CHUNK = 65536                                             # points per call of the device entry (bounds the device memory of the outputs)


def _chain_parts(samples):
    """(kind, chains): the chain(s) in what a sampler, ``sampler.chains``, ``sampler.chain``, a :class:`Samples`, a dict or a ``ChainFile`` gives."""
    from .io import ChainFile
    if isinstance(samples, ChainFile):
        return 'chainfile', [samples]
    if isinstance(samples, dict):
        return 'samples', [samples]
    if hasattr(samples, 'chains') and not hasattr(samples, 'keys'):   # a sampler
        samples = samples.chains
    chains = [chain for chain in samples if chain is not None]
    if not chains:
        raise ValueError('sample_solved: no samples (the sampler has not run yet)')
    return 'list', chains


def sample_solved(likelihood, samples, size=1, seed=42):
    """
    Sample the parameters that have been marginalised analytically (samples/chain.py:229-263).

    Parameters
    ----------
    likelihood : ObservablesGaussianLikelihood
        The likelihood the chain was sampled from (its '.marg' / '.best' / '.auto' parameters are drawn; '.prec' parameters are not).
    samples : dict, Samples, ChainFile, sampler, list
        name -> array of any shape holding at least the sampled parameters: ``sampler.chain`` / an entry of ``sampler.chains`` of any sampler of this
        package, a :class:`Samples`, a ``ChainFile``; or a sampler / ``sampler.chains`` (every chain is treated; a list is returned).
    size : int, default=1
        Draws per chain point.
    seed : int, default=42
        Key of the counter-based draws: draw ``d`` of component ``s`` at point ``i`` is a pure function of (seed, i, d, s), ``i`` the index of the point in the
        flattened chain (chains of a list one after the other).

    Returns
    -------
    new : Samples, ChainFile, list
        Every array repeated ``size`` times along the last axis (weights -- 'aweight', 'fweight', the 'logweight' of SMC / nested chains -- unchanged, chain.py:244-245), the solved parameters as ordinary columns holding the draws,
        ``loglikelihood``, ``logprior`` and ``logposterior`` replaced by the values with nothing marginalised.  Points whose evaluation fails keep NaN.
    """
    from .io import ChainFile
    size = int(size)
    if size < 1:
        raise ValueError('sample_solved: size must be at least 1, found {:d}'.format(size))
    if hasattr(likelihood, 'initialize'): likelihood.initialize()
    varied, solved = list(likelihood.varied_params), list(likelihood.solved_params)
    if not solved:
        raise ValueError('sample_solved: the likelihood has no analytically solved parameter')
    ctx = likelihood._get_context()
    if ctx.n_solved != len(solved):
        raise ValueError('sample_solved: the context solves {:d} parameters, the likelihood {:d}'.format(ctx.n_solved, len(solved)))
    ll_name, lp_name = str(getattr(likelihood, '_param_loglikelihood', 'loglikelihood')), str(getattr(likelihood, '_param_logprior', 'logprior'))
    kind, chains = _chain_parts(samples)
    out, index0, nbad = [], 0, 0
    for chain in chains:
        arrays = dict(chain.to_samples()) if isinstance(chain, ChainFile) else {str(name): np.asarray(value) for name, value in chain.items()}
        missing = [param.name for param in varied if param.name not in arrays]
        if missing:
            raise ValueError('sample_solved: the samples lack the sampled parameters {}'.format(missing))
        shape = np.shape(arrays[varied[0].name])
        if len(shape) == 0:
            raise ValueError('sample_solved: samples must be arrays of at least one dimension')
        theta = np.column_stack([np.ravel(arrays[param.name]) for param in varied]).astype('f8')
        npoints = theta.shape[0]
        x = np.empty((npoints, size, len(solved)), dtype='f8')
        loglike, logprior = np.empty((npoints, size), dtype='f8'), np.empty((npoints, size), dtype='f8')
        for start in range(0, npoints, CHUNK):
            piece = ctx.sample_solved(theta[start:start + CHUNK], index0=index0 + start, size=size, seed=seed)
            x[start:start + CHUNK], loglike[start:start + CHUNK], logprior[start:start + CHUNK] = piece[:3]
            nbad += int(np.count_nonzero(piece[3]))
        index0 += npoints
        new_shape = shape[:-1] + (shape[-1] * size,)
        new = {}
        for name, value in arrays.items():
            if name.startswith(ll_name + '.') or name.startswith(lp_name + '.'): continue   # Hessian entries w.r.t. the solved parameters: dropped (derivs=None, chain.py:255)
            new[name] = np.repeat(value, size, axis=len(shape) - 1) if np.shape(value) == shape else value
        for iparam, param in enumerate(solved):
            new[param.name] = x[..., iparam].reshape(new_shape)
        new[ll_name], new[lp_name] = loglike.reshape(new_shape), logprior.reshape(new_shape)
        new['logposterior'] = new[ll_name] + new[lp_name]
        out.append(new)
    if nbad:
        warnings.warn('sample_solved: {:d} chain points could not be evaluated (outside the prior, NaN input or a non-finite likelihood): their solved '
                      'parameters, loglikelihood, logprior and logposterior are NaN'.format(nbad))
    if kind == 'chainfile':
        source = chains[0]
        all_params = dict(source.params)
        all_params.update({param.name: param.clone(derived=False) for param in solved})   # ordinary columns from now on (chain.py:250)
        return ChainFile(out[0], params=all_params, attrs=source.attrs)   # (zero-lag values: the derivatives w.r.t. the solved parameters are consumed here)
    out = [Samples(new) for new in out]
    return out[0] if kind == 'samples' else out
