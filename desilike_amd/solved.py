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


def _chain_arrays(chain, varied):
    """(arrays, shape, theta [npoints, n_varied]) of one chain."""
    from .io import ChainFile
    arrays = dict(chain.to_samples()) if isinstance(chain, ChainFile) else {str(name): np.asarray(value) for name, value in chain.items()}
    missing = [param.name for param in varied if param.name not in arrays]
    if missing:
        raise ValueError('sample_solved: the samples lack the sampled parameters {}'.format(missing))
    shape = np.shape(arrays[varied[0].name])
    if len(shape) == 0:
        raise ValueError('sample_solved: samples must be arrays of at least one dimension')
    return arrays, shape, np.column_stack([np.ravel(arrays[param.name]) for param in varied]).astype('f8')


def _new_chain(arrays, shape, size, solved, x, loglike, logprior, ll_name, lp_name):
    """The chain with every array repeated ``size`` times along the last axis, the draws ``x [npoints, size, n_solved]`` and the corrected values."""
    new_shape = shape[:-1] + (shape[-1] * size,)
    new = {}
    for name, value in arrays.items():
        if name.startswith(ll_name + '.') or name.startswith(lp_name + '.'): continue   # Hessian entries w.r.t. the solved parameters: dropped (derivs=None, chain.py:255)
        new[name] = np.repeat(value, size, axis=len(shape) - 1) if np.shape(value) == shape else value
    for iparam, param in enumerate(solved):
        new[param.name] = x[..., iparam].reshape(new_shape)
    new[ll_name], new[lp_name] = loglike.reshape(new_shape), logprior.reshape(new_shape)
    new['logposterior'] = new[ll_name] + new[lp_name]
    return new


def _warn_bad(nbad):
    if nbad:
        warnings.warn('sample_solved: {:d} chain points could not be evaluated (outside the prior, NaN input or a non-finite likelihood): their solved '
                      'parameters, loglikelihood, logprior and logposterior are NaN'.format(nbad))


POINT_ADVICE = "the solved parameters of a data batch are available with data_batch(data, solve='point')"


def check_point_batch(data_batch):
    """The data batch draws can be taken from: made with ``solve='point'``."""
    if getattr(data_batch, 'solve', None) != 'point':
        raise ValueError(POINT_ADVICE)
    return data_batch


def sample_solved_chains(data_batch, chains, index, size=1, seed=42):
    """The data-batch form of :func:`sample_solved` on a list of chains, chain c against data vector ``index[c]``: all chains are flattened into ONE point list with a
    data index per point -- chain after chain, each in its own flattening; that order is the global point index of the draws -- and treated in calls of ``CHUNK``
    points, whatever the number of chains or of data vectors.  Returns the list of new chains (dicts)."""
    likelihood = data_batch.likelihood
    varied, solved = list(likelihood.varied_params), list(likelihood.solved_params)
    ll_name, lp_name = str(getattr(likelihood, '_param_loglikelihood', 'loglikelihood')), str(getattr(likelihood, '_param_logprior', 'logprior'))
    parts = [_chain_arrays(chain, varied) for chain in chains]
    if not parts:
        return []
    theta = np.concatenate([part[2] for part in parts])
    counts = [part[2].shape[0] for part in parts]
    point_index = np.repeat(np.asarray(index, dtype='i4'), counts)
    npoints = theta.shape[0]
    x = np.empty((npoints, size, len(solved)), dtype='f8')
    loglike, logprior = np.empty((npoints, size), dtype='f8'), np.empty((npoints, size), dtype='f8')
    nbad = 0
    for start in range(0, npoints, CHUNK):
        piece = data_batch.sample_solved(theta[start:start + CHUNK], point_index[start:start + CHUNK], index0=start, size=size, seed=seed)
        x[start:start + CHUNK], loglike[start:start + CHUNK], logprior[start:start + CHUNK] = piece[:3]
        nbad += int(np.count_nonzero(piece[3]))
    _warn_bad(nbad)
    out, start = [], 0
    for (arrays, shape, _), count in zip(parts, counts):
        sl = slice(start, start + count)
        out.append(_new_chain(arrays, shape, size, solved, x[sl], loglike[sl], logprior[sl], ll_name, lp_name))
        start += count
    return out


def _chain_index(index, kind, samples, data_batch):
    """One data vector per chain (``None`` entries of a list dropped with their chains): an int for a single chain, a sequence for a list."""
    if index is None:
        raise ValueError('sample_solved: index is required with a data batch: the data vector of every chain (an int for one chain, a sequence for a list)')
    index = np.asarray(index)
    if not np.issubdtype(index.dtype, np.integer):
        raise ValueError('sample_solved: index must hold integers, found type {}'.format(index.dtype))
    if kind != 'list':
        if index.size != 1:
            raise ValueError('sample_solved: index must be one integer for a single chain, found shape {}'.format(index.shape))
        index = index.reshape(1)
    else:
        if hasattr(samples, 'chains') and not hasattr(samples, 'keys'): samples = samples.chains
        keep = [chain is not None for chain in samples]
        if index.shape != (len(keep),):
            raise ValueError('sample_solved: index must be one integer per chain ({:d}), found shape {}'.format(len(keep), index.shape))
        index = index[np.array(keep, dtype=bool)]
    if index.size and (index.min() < 0 or index.max() >= data_batch.size):
        raise ValueError('sample_solved: index must lie in [0, {:d})'.format(data_batch.size))
    return index


def sample_solved(likelihood, samples, size=1, seed=42, index=None):
    """
    Sample the parameters that have been marginalised analytically (samples/chain.py:229-263).

    Parameters
    ----------
    likelihood : ObservablesGaussianLikelihood, DataBatch
        The likelihood the chain was sampled from (its '.marg' / '.best' / '.auto' parameters are drawn; '.prec' parameters are not); or a data batch made with
        ``likelihood.data_batch(data, solve='point')``: every chain is then taken against ONE data vector of the batch, named by ``index``.
    samples : dict, Samples, ChainFile, sampler, list
        name -> array of any shape holding at least the sampled parameters: ``sampler.chain`` / an entry of ``sampler.chains`` of any sampler of this
        package, a :class:`Samples`, a ``ChainFile``; or a sampler / ``sampler.chains`` (every chain is treated; a list is returned).
    size : int, default=1
        Draws per chain point.
    seed : int, default=42
        Key of the counter-based draws: draw ``d`` of component ``s`` at point ``i`` is a pure function of (seed, i, d, s), ``i`` the index of the point in the
        flattened chain (chains of a list one after the other).
    index : int, sequence of int, default=None
        With a data batch (required): the data vector of every chain -- an int for a single chain, one int per chain for a list.  Not accepted with a likelihood.

    Returns
    -------
    new : Samples, ChainFile, list
        Every array repeated ``size`` times along the last axis (weights -- 'aweight', 'fweight', the 'logweight' of SMC / nested chains -- unchanged, chain.py:244-245), the solved parameters as ordinary columns holding the draws,
        ``loglikelihood``, ``logprior`` and ``logposterior`` replaced by the values with nothing marginalised.  Points whose evaluation fails keep NaN.
    """
    from .likelihoods.base import DataBatch
    size = int(size)
    if size < 1:
        raise ValueError('sample_solved: size must be at least 1, found {:d}'.format(size))
    data_batch = None
    if isinstance(likelihood, DataBatch):
        data_batch, likelihood = check_point_batch(likelihood), likelihood.likelihood
    elif index is not None:
        raise ValueError('sample_solved: index names the data vectors of a data batch; pass likelihood.data_batch(data, solve=\'point\') as the first argument')
    if hasattr(likelihood, 'initialize'): likelihood.initialize()
    varied, solved = list(likelihood.varied_params), list(likelihood.solved_params)
    if not solved:
        raise ValueError('sample_solved: the likelihood has no analytically solved parameter')
    ctx = data_batch.context if data_batch is not None else likelihood._get_context()
    if ctx.n_solved != len(solved):
        raise ValueError('sample_solved: the context solves {:d} parameters, the likelihood {:d}'.format(ctx.n_solved, len(solved)))
    ll_name, lp_name = str(getattr(likelihood, '_param_loglikelihood', 'loglikelihood')), str(getattr(likelihood, '_param_logprior', 'logprior'))
    kind, chains = _chain_parts(samples)
    if data_batch is not None:
        out = sample_solved_chains(data_batch, chains, _chain_index(index, kind, samples, data_batch), size=size, seed=seed)
        return _finish(kind, chains, out, solved)
    out, index0, nbad = [], 0, 0
    for chain in chains:
        arrays, shape, theta = _chain_arrays(chain, varied)
        npoints = theta.shape[0]
        x = np.empty((npoints, size, len(solved)), dtype='f8')
        loglike, logprior = np.empty((npoints, size), dtype='f8'), np.empty((npoints, size), dtype='f8')
        for start in range(0, npoints, CHUNK):
            piece = ctx.sample_solved(theta[start:start + CHUNK], index0=index0 + start, size=size, seed=seed)
            x[start:start + CHUNK], loglike[start:start + CHUNK], logprior[start:start + CHUNK] = piece[:3]
            nbad += int(np.count_nonzero(piece[3]))
        index0 += npoints
        out.append(_new_chain(arrays, shape, size, solved, x, loglike, logprior, ll_name, lp_name))
    _warn_bad(nbad)
    return _finish(kind, chains, out, solved)


def _finish(kind, chains, out, solved):
    from .io import ChainFile
    if kind == 'chainfile':
        source = chains[0]
        all_params = dict(source.params)
        all_params.update({param.name: param.clone(derived=False) for param in solved})   # ordinary columns from now on (chain.py:250)
        return ChainFile(out[0], params=all_params, attrs=source.attrs)   # (zero-lag values: the derivatives w.r.t. the solved parameters are consumed here)
    out = [Samples(new) for new in out]
    return out[0] if kind == 'samples' else out
