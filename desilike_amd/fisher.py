"""Fisher matrix of a Gaussian likelihood (reference: desilike/fisher.py:642-809, 63-640; differentiation.py).

``Fisher(likelihood)(**center)`` evaluates the theory vector on the whole finite-difference stencil of the varied parameters as ONE GPU
batch (the reference's ``Differentiation`` scatters the stencil points over MPI ranks, differentiation.py:394-398) and ``dl_eval_fisher``
(csrc/dl_fisher.hip) forms ``d(flatdiff)/d(theta)`` by central differences of step ``Parameter.delta`` (or, ``method='analytic'``, takes it exactly from the
theory's Jacobian kernel, csrc/dl_fullshape_jac.h, or from the forward mode of an emulated PT node, csrc/dl_emu_jac.h: ``dl_eval_fisher_analytic``) and the reference's Gaussian finalisation
(fisher.py:731-750) on the device: ``hessian = -dD P dD^T``, ``gradient = -dD P D``, ``offset = -D P D`` (no 1/2, as in the reference, line 746).
The host adds the Gaussian prior terms (fisher.py:706-716) and keeps the P x P ``LikelihoodFisher`` algebra (216-257).
"""
import numpy as np


class LikelihoodFisher(object):
    """Gaussian approximation of a likelihood around ``center`` (fisher.py:63-640, the parts the hot path produces / consumes)."""

    def __init__(self, center, params, offset=0., gradient=None, hessian=None, with_prior=False):
        self._center = np.asarray(center, dtype='f8')
        self._params = list(params)
        n = self._center.size
        self._offset = float(offset)
        self._gradient = np.zeros(n) if gradient is None else np.asarray(gradient, dtype='f8')
        self._hessian = np.zeros((n, n)) if hessian is None else np.asarray(hessian, dtype='f8')
        self.with_prior = bool(with_prior)

    def names(self):
        return [str(param) for param in self._params]

    def _solve(self):
        return np.linalg.solve(self._hessian, self._gradient)   # fisher.py:216-221

    @property
    def chi2min(self):
        flatdiff = -self._solve()   # fisher.py:224-227
        return -2. * (self._offset + self._gradient.dot(flatdiff) + 0.5 * flatdiff.dot(self._hessian).dot(flatdiff))

    def mean(self):
        return self._center - self._solve()   # fisher.py:229-243

    def center(self):
        return self._center.copy()

    def precision(self):
        return -self._hessian

    def covariance(self):
        return np.linalg.inv(-self._hessian)

    def std(self):
        return np.diag(self.covariance())**0.5

    def __add__(self, other):
        """Sum of independent Gaussian likelihoods expanded around the same centre."""
        assert self.names() == other.names() and np.allclose(self._center, other._center)
        return LikelihoodFisher(self._center, self._params, self._offset + other._offset, self._gradient + other._gradient, self._hessian + other._hessian,
                                with_prior=self.with_prior or other.with_prior)

    def to_likelihood(self):
        return FisherGaussianLikelihood(self)


class FisherGaussianLikelihood(object):
    """Gaussian-in-parameters likelihood built from a :class:`LikelihoodFisher` (likelihoods/galaxy_clustering/fisher.py:31-60 / fisher.py 'to_likelihood'):
    ``loglikelihood(theta) = offset + g (theta - c) + 1/2 (theta - c) H (theta - c)``."""

    def __init__(self, fisher):
        self.fisher = fisher

    def __call__(self, **params):
        diff = np.array([params[name] for name in self.fisher.names()]) - self.fisher._center
        return self.fisher._offset + self.fisher._gradient.dot(diff) + 0.5 * diff.dot(self.fisher._hessian).dot(diff)


class Fisher(object):
    """Estimate the Fisher matrix of ``likelihood`` (a Gaussian likelihood of this package) entirely on the GPU.  ``method='finite'`` (default): the stencil of all
    centres goes through the theory kernels and the whitened window GEMM as one batch and ``dl_eval_fisher`` forms ``offset``, ``gradient`` and ``hessian``
    (fisher.py:739-748) with an fp64 MFMA Gram product per centre.  ``method='analytic'``: ``dl_eval_fisher_analytic`` -- the same algebra on EXACT derivative rows
    written by the theory's Jacobian kernel (csrc/dl_fullshape_jac.h; what the reference's ``Differentiation`` takes from jax) or, for one velocileptors observable on an
    MLP- / Taylor-emulated PT node, by the forward mode through the emulator and the bias monomials (csrc/dl_emu_jac.h): no step size, one theory row per centre
    instead of 1 + 2 P; ``NotImplementedError`` outside its scope (:attr:`SCOPE`).  ``'auto'``: analytic where available AND measured faster than the stencil
    (Kaiser likelihoods: DESIGN.md section 6d; emulated ones: :attr:`AUTO_EMULATED`), else finite.

    Analytically solved parameters ('.marg' / '.best' / '.auto' / '.prec') are VARIED, as in the reference, which warns and works on a copy of the likelihood with
    ``derived=False`` for them (fisher.py:688-695)."""

    SCOPE = ('the analytic Fisher covers Kaiser full-shape likelihoods (fixed / ShapeFit template on uniform knots, no damping, no counter terms, no pass-through '
             'columns, no observable transform; any number of observables; at most 31 parameters) and ONE velocileptors P_ell observable on an emulated PT node '
             '(table engine an MLP or a Taylor engine, sigma8 / fsigma8 engines MLP, Taylor or constant; not the stacked layout, not xi_ell, no transform; at most '
             '31 parameters, the solved ones included): use method="finite"')
    AUTO_EMULATED = False     # whether 'auto' takes the analytic path on an emulated context: set from the measurement of DESIGN.md section 6f

    def __init__(self, likelihood, delta_scale=1., method='finite'):
        if method not in ('finite', 'analytic', 'auto'): raise ValueError('method must be one of finite, analytic, auto')
        self.method = method
        self.likelihood = likelihood
        likelihood.initialize()
        self.delta_scale = float(delta_scale)
        solved = [param for param in likelihood.all_params if param.solved]
        if solved:
            import warnings
            warnings.warn('solved parameters: {}; cannot proceed with solved parameters, so they are varied in the Fisher estimate'.format([param.name for param in solved]))
        from .parameter import ParameterCollection
        self.varied_params = ParameterCollection(list(likelihood.varied_params) + solved)
        self._solved_names = [param.name for param in solved]
        self._ctx = None
        self._data_ctx = None

    def set_data_batch(self, data):
        """Give the Fisher context the data vectors ``data`` (array ``[M, n_data]`` in ``flatdata`` order, or a list of per-observable arrays: ``likelihood.data_batch``)
        for :meth:`evaluate` with ``data_index``; ``None`` drops them.  The context that holds them is a private one: the likelihood's own is shared with its samplers.
        Returns the number of data vectors."""
        if data is None:
            if self._data_ctx is not None: self._data_ctx.close()
            self._data_ctx = None
            return 0
        from ._lib import Context, check_data_batch
        from .likelihoods.base import flatten_data_batch
        like = getattr(self.likelihood, '_fused', self.likelihood)
        sizes = [obs.wmatrix.size for obs in like.observables]
        flatdata = check_data_batch(flatten_data_batch(data, sizes), sum(sizes))      # (before any device call)
        if self._data_ctx is None:
            # every solved and '.prec' parameter is varied here: the configuration holds the likelihood's data vector as it is, nothing to add to the batch
            self._data_ctx = Context(like._spec({}, like._flatdata_list(), like._precision_input, vary_solved=bool(self._solved_names)), device=like.device)
        return self._data_ctx.set_data_batch(flatdata)

    def _get_context(self):
        if self._ctx is None:
            like = self.likelihood
            if self._solved_names:
                from ._lib import Context
                self._ctx = Context(like._spec({}, like._flatdata_list(), like._precision_input, vary_solved=True), device=like.device)
            else:
                self._ctx = like._get_context()
        return self._ctx

    def steps(self, centers):
        """Lower / upper finite-difference steps ``[B, P, 2]`` at ``centers [B, P]``: ``Parameter.delta`` = (value, step below, step above) (parameter.py:898-915)
        scaled by ``delta_scale``, shortened where a prior bound is closer."""
        centers = np.atleast_2d(centers)
        steps = np.empty(centers.shape + (2,), dtype='f8')
        for ip, param in enumerate(self.varied_params):
            _, lower, upper = param.delta
            steps[:, ip, 0] = np.minimum(lower * self.delta_scale, centers[:, ip] - param.prior.limits[0])
            steps[:, ip, 1] = np.minimum(upper * self.delta_scale, param.prior.limits[1] - centers[:, ip])
        if not (steps.sum(axis=-1) > 0.).all():
            raise ValueError('zero finite-difference interval: a centre sits on both prior bounds of a parameter')
        return np.clip(steps, 0., None)

    def evaluate(self, centers, data_index=None):
        """``centers [B, P]`` (columns ordered as :attr:`varied_params`) -> (offset [B], gradient [B, P], hessian [B, P, P]) of the likelihood term, one GPU batch.
        ``data_index [B]``: centre b against data vector ``data_index[b]`` of :meth:`set_data_batch` -- ``method='analytic'``: ``dl_eval_fisher_analytic_data``
        (``NotImplementedError`` outside :attr:`SCOPE`); ``'finite'`` and ``'auto'``: ``dl_eval_fisher_data``, the finite-difference route."""
        import torch
        centers = np.ascontiguousarray(np.atleast_2d(centers), dtype='f8')
        if data_index is not None:
            if self._data_ctx is None: raise ValueError('no data batch: call set_data_batch first')
            data_index = np.asarray(data_index)
            if data_index.shape != (centers.shape[0],) or not np.issubdtype(data_index.dtype, np.integer):
                raise ValueError('data_index must be {:d} integers'.format(centers.shape[0]))
            ctx = self._data_ctx
            device = torch.device('cuda', ctx.device)
            index = torch.as_tensor(np.ascontiguousarray(data_index, dtype='i4'), device=device)
            if self.method == 'analytic':
                out = ctx.eval_fisher_analytic_data(torch.as_tensor(centers, device=device), index)   # (None: outside the Jacobian kernels' scope, the context decides)
                if out is None: raise NotImplementedError(self.SCOPE)
                hessian, gradient, offset = out
                return offset.cpu().numpy(), gradient.cpu().numpy(), hessian.cpu().numpy()
            hessian, gradient, offset = ctx.eval_fisher_data(torch.as_tensor(centers, device=device), torch.as_tensor(self.steps(centers), device=device).contiguous(), index)
            return offset.cpu().numpy(), gradient.cpu().numpy(), hessian.cpu().numpy()
        ctx = self._get_context()
        device = torch.device('cuda', ctx.device)
        if self.method == 'analytic' or (self.method == 'auto' and (self.AUTO_EMULATED or not getattr(ctx, 'emulated', False))):
            # exact derivative rows (dl_eval_fisher_analytic): no steps, one theory row per centre; None: outside the Jacobian kernels' scope, the context decides
            out = ctx.eval_fisher_analytic(torch.as_tensor(centers, device=device))
            if out is not None:
                hessian, gradient, offset = out
                return offset.cpu().numpy(), gradient.cpu().numpy(), hessian.cpu().numpy()
            if self.method == 'analytic': raise NotImplementedError(self.SCOPE)
        hessian, gradient, offset = ctx.eval_fisher(torch.as_tensor(centers, device=device), torch.as_tensor(self.steps(centers), device=device).contiguous())
        return offset.cpu().numpy(), gradient.cpu().numpy(), hessian.cpu().numpy()

    def __call__(self, **params):
        varied = self.varied_params
        center = np.array([params.get(param.name, param.value) for param in varied], dtype='f8')
        offset, gradient, hessian = (array[0] for array in self.evaluate(center[None, :]))
        likelihood_fisher = LikelihoodFisher(center, varied, offset=offset, gradient=gradient, hessian=hessian)
        # Gaussian priors (fisher.py:706-716)
        poffset, pgradient, phessian = 0., [], []
        for param, value in zip(varied, center):
            loc, scale = (param.prior.loc, param.prior.scale) if param.prior.dist == 'norm' else (0., np.inf)
            prec = scale**(-2)
            poffset += -0.5 * (value - loc)**2 * prec
            pgradient.append(-(value - loc) * prec)
            phessian.append(-prec)
        prior_fisher = LikelihoodFisher(center, varied, offset=poffset, gradient=pgradient, hessian=np.diag(phessian), with_prior=True)
        self.likelihood_fisher, self.prior_fisher = likelihood_fisher, prior_fisher
        return likelihood_fisher + prior_fisher


def logposterior_value_and_grad(likelihood, theta, method='auto'):
    r"""Log-posterior and its gradient w.r.t. the varied parameters for a batch of points.

    ``method='analytic'``: ``dl_eval_logposterior_grad`` -- the gradient is formed on the device from the theory's own derivatives (csrc/dl_fullshape_grad.h:
    one forward pass, one extra GEMM, one gradient pass: about 2.5 evaluations instead of 2 P + 1), for Kaiser full-shape likelihoods with uniform / Gaussian priors,
    and one MLP-emulated velocileptors observable with solved parameters (csrc/dl_emu_grad.h);
    ``'finite'``: central differences evaluated as ONE GPU batch (below); ``'auto'``: analytic where the context supports it, else central differences.

    What gradient-based samplers ask of the likelihood (``jax.value_and_grad(logposterior)``: desilike/samplers/hmc.py:194, nuts.py:205, mclmc.py); the reference
    obtains it from jax tracing, here the stencil ``theta_b \pm h_p e_p`` of all B points and P parameters (B (2 P + 1) rows) goes through ``dl_eval_logposterior``
    in one call.  Steps are ``Parameter.delta`` (parameter.py:898-915), shortened where a prior bound is closer (one-sided there).  Analytically solved parameters
    are marginalised inside every evaluation.  Returns ``(logposterior [B], gradient [B, P])``; rows outside the prior get ``-inf`` and a NaN gradient.
    """
    import torch
    if method not in ('auto', 'analytic', 'finite'): raise ValueError('method must be one of auto, analytic, finite')
    likelihood.initialize()
    varied = likelihood.varied_params
    theta = np.atleast_2d(np.asarray(theta, dtype='f8'))
    B, P = theta.shape
    assert P == len(varied)
    if method != 'finite':
        ctx = likelihood._get_context()
        th = torch.as_tensor(theta, dtype=torch.float64, device=torch.device('cuda', ctx.device)).contiguous()
        out = ctx.eval_logposterior_grad(th)   # (None: outside the analytic gradient's scope, the context decides)
        if out is not None:
            return out[0].cpu().numpy(), out[1].cpu().numpy()
        if method == 'analytic':
            raise NotImplementedError('the analytic gradient covers Kaiser full-shape likelihoods (uniform template knots, no counter terms, no damping, no transform, no solved '
                                      'parameters) and one MLP-emulated velocileptors observable (solved parameters allowed), with uniform / norm priors: use method="finite"')
    lower, upper = np.empty((B, P)), np.empty((B, P))
    for ip, param in enumerate(varied):
        _, lo, hi = param.delta
        lower[:, ip] = np.clip(np.minimum(lo, theta[:, ip] - param.prior.limits[0]), 0., None)
        upper[:, ip] = np.clip(np.minimum(hi, param.prior.limits[1] - theta[:, ip]), 0., None)
    points = np.repeat(theta[:, None, :], 2 * P + 1, axis=1)                 # [B, 1 + 2 P, P]
    index = np.arange(P)
    points[:, 1 + 2 * index, index] -= lower
    points[:, 2 + 2 * index, index] += upper
    ctx = likelihood._get_context()
    device = torch.device('cuda', ctx.device)
    pts = torch.as_tensor(points.reshape(-1, P), dtype=torch.float64, device=device).contiguous()
    out = torch.empty(pts.shape[0], dtype=torch.float64, device=device)
    ctx.eval_logposterior(pts, out)
    logpost = out.cpu().numpy().reshape(B, 2 * P + 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        gradient = (logpost[:, 2::2] - logpost[:, 1::2]) / (lower + upper)
    return logpost[:, 0], gradient
