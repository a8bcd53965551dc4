"""Gradient oracle of the emulated full-shape likelihoods: a torch (float64, CPU) restatement of the NumPy oracle chain of ``bench_configs.cfg3_oracle_solution`` /
``test_gpu_emulator.oracle_flat`` -- ``mlp_predict`` -> ``velocileptors_pars`` -> ``tablevel_combine_bias_terms_poles`` -> ``interp1d`` -> ``window_apply`` ->
``solve_marginalized`` (with its slogdet) -- differentiated by autograd.  The reference takes the same derivative with ``jax.value_and_grad``
(desilike/samplers/hmc.py:194), which is not available here.  The cubic interpolation is linear in the tabulated values: it enters as the matrix the NumPy oracle's
``interp1d`` makes of the identity, so both sides share it exactly."""
import numpy as np
import torch

from oracle import np_oracle as orc

VPARS = ['b1p', 'b2p', 'bsp', 'b3p', 'alpha0p', 'alpha2p', 'alpha4p', 'sn0p', 'sn2p', 'sn4p']


def _act(v, activation):
    if activation == 'silu': return v / (1. + torch.exp(-v))
    if activation == 'relu': return torch.clamp(v, min=0.)
    if activation == 'tanh': return torch.tanh(v)
    raise ValueError(activation)


def mlp_predict(x, engine):
    """orc.mlp_predict in torch: x [P] tensor."""
    xl = torch.as_tensor(np.array(engine.xlimits, dtype='f8'))
    v = (x - xl[..., 0]) / (xl[..., 1] - xl[..., 0])
    for ilayer, (kernel, bias) in enumerate(engine.layers):
        v = v @ torch.as_tensor(np.asarray(kernel, dtype='f8')) + torch.as_tensor(np.asarray(bias, dtype='f8'))
        if ilayer < len(engine.layers) - 1: v = _act(v, engine.activation)
    yl = torch.as_tensor(np.array(engine.ylimits, dtype='f8'))
    return v * (yl[..., 1] - yl[..., 0]) + yl[..., 0]


def velocileptors_pars(params, sigma8, f, model, snd, fsat, sigv):
    """orc.velocileptors_pars, physical basis."""
    b1L, b2L, bsL, b3L = params['b1p'] / sigma8 - 1., params['b2p'] / sigma8**2, params['bsp'] / sigma8**2, params['b3p'] / sigma8**3
    pars = [1. + b1L, 8. / 21. * b1L + b2L, bsL, b3L] if model == 'rept' else [b1L, b2L, bsL, b3L]
    pars += [(1 + b1L)**2 * params['alpha0p'], f * (1 + b1L) * (params['alpha0p'] + params['alpha2p']),
             f * (f * params['alpha2p'] + (1 + b1L) * params['alpha4p']), f**2 * params['alpha4p']]
    pars += [params['sn{:d}p'.format(i)] * snd * (fsat if i > 0 else 1.) * sigv**i for i in [0, 2, 4]]
    if model == 'rept':
        b1 = pars[0]
        pars[2] = pars[2] - (2 / 7) * (b1 - 1.)
        pars[3] = 3 * pars[3] + (b1 - 1.)
    return pars


def monomials(pars, nd):
    b1, b2, bs, b3, alpha0, alpha2, alpha4, alpha6, sn0, sn2, sn4 = pars
    one = torch.ones((), dtype=torch.float64)
    return torch.stack([one * v for v in [1., b1, b1**2, b2, b1 * b2, b2**2, bs, b1 * bs, b2 * bs, bs**2, b3, b1 * b3, alpha0, alpha2, alpha4, alpha6, sn0 / nd, sn2 / nd, sn4 / nd]])


class EmulatedOracle(object):
    """Log-posterior of an emulated likelihood at one point of its varied parameters, as a torch function (``value_and_grad``)."""

    def __init__(self, like, pt, theory, solved, in_params, model, kinds=None):
        self.like, self.pt, self.theory, self.solved, self.in_params, self.model = like, pt, theory, list(solved), list(in_params), model
        self.names = like.varied_params.names()
        self.kinds = kinds or {name: '.marg' for name in self.solved}
        self.interp = torch.as_tensor(orc.interp1d(theory.k, pt.k, np.eye(len(pt.k))))               # [n_kin, n_k]: the cubic interpolation as a matrix
        wm = like.observables[0].wmatrix
        self.wfull = torch.as_tensor(np.asarray(wm.matrix_full, dtype='f8'))
        self.snin = torch.as_tensor(np.asarray(wm.shotnoisein, dtype='f8'))
        self.snout = torch.as_tensor(np.asarray(wm.shotnoiseout, dtype='f8'))
        self.data = torch.as_tensor(np.asarray(like.flatdata, dtype='f8'))
        self.precision = torch.as_tensor(np.asarray(like.precision, dtype='f8'))
        self.scales = np.array([like.all_params[name].prior.scale for name in self.solved], dtype='f8')
        self.priors = [(param.prior.dist, getattr(param.prior, 'loc', 0.), getattr(param.prior, 'scale', 1.)) for param in like.varied_params]

    def flat(self, p):
        eng = self.pt.engines
        xin = torch.stack([torch.as_tensor(p[name], dtype=torch.float64) for name in self.in_params])
        pktable = mlp_predict(xin, eng['pktable']).reshape(3, -1, 19)
        sigma8 = mlp_predict(xin, eng['sigma8'])[0]
        fsigma8 = mlp_predict(xin, eng['fsigma8'])[0]
        params = {name: p.get(name, self.like.all_params[name].value) for name in VPARS}
        th = self.theory
        pars = velocileptors_pars(params, sigma8, fsigma8 / sigma8, self.model, th.snd, th.fsat, th.sigv)
        table = pktable @ monomials(pars, th.nd)                   # [3, n_k]
        power = table @ self.interp.T                              # [3, n_kin]
        return self.wfull @ torch.ravel(power + self.snin[:, None]) - self.snout

    def logposterior(self, theta):
        """theta: [P] float64 tensor (may require grad) -> scalar tensor (log-likelihood + solved priors + priors of theta)."""
        p = {name: theta[i] for i, name in enumerate(self.names)}
        nsol = len(self.solved)
        f0 = self.flat(dict(p, **{name: 0. for name in self.solved}))
        diff = f0 - self.data
        ll = -0.5 * diff @ self.precision @ diff
        lp = torch.zeros((), dtype=torch.float64)
        if nsol:
            # the theory is linear in the solved parameters: derivative rows from unit vectors through the same chain
            T = torch.stack([self.flat(dict(p, **{n2: float(n2 == name) for n2 in self.solved})) - f0 for name in self.solved])
            derivp = T @ self.precision
            lgrad = -derivp @ diff
            lhess = -derivp @ T.T
            prec = torch.as_tensor(self.scales**(-2))
            phess = -torch.diag(prec) + lhess
            dx = -torch.linalg.solve(phess, lgrad)                 # x0 = prior loc = 0
            ll = ll + 0.5 * dx @ lhess @ dx + lgrad @ dx
            lp = lp + torch.sum(-0.5 * dx**2 * prec)
            marg = np.array([self.kinds[name] == '.marg' for name in self.solved])
            if marg.any():
                idx = torch.as_tensor(np.flatnonzero(marg))
                ll = ll - 0.5 * torch.linalg.slogdet(-phess[idx][:, idx])[1]
        for i, (dist, loc, scale) in enumerate(self.priors):
            if dist == 'norm': lp = lp - 0.5 * ((theta[i] - loc) / scale)**2
        return ll + lp

    def value_and_grad(self, row):
        theta = torch.tensor(np.asarray(row, dtype='f8'), requires_grad=True)
        value = self.logposterior(theta)
        (grad,) = torch.autograd.grad(value, theta)
        return float(value.detach()), grad.numpy()
