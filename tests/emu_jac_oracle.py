"""Jacobian oracle of the emulated full-shape likelihoods: the torch chain of ``emu_grad_oracle.EmulatedOracle`` (left as it is) with every solved parameter varied, as
``Fisher`` varies them, a torch ``taylor_predict`` beside ``mlp_predict``, and ``J = torch.autograd.functional.jacobian`` of the theory vector -- exact, no step.  From it
the Fisher algebra of fisher.py:739-748: ``hessian_ref = -J^T P J``, ``gradient_ref = -J^T P (flat - data)`` and ``offset_ref = -1/2 (flat - data)^T P (flat - data)``, the
log-likelihood.  The device keeps the reference's convention for the offset (``-(flat - data)^T P (flat - data)``, no 1/2: fisher.py:746), so HALF the device's offset is
compared with ``offset_ref``."""
import numpy as np
import torch

from emu_grad_oracle import EmulatedOracle, VPARS, mlp_predict, velocileptors_pars, monomials


def taylor_predict(x, engine):
    """orc.taylor_predict in torch: x [P] tensor -> [*yshape]."""
    dx = x - torch.as_tensor(np.asarray(engine.center, dtype='f8'))
    powers = np.asarray(engine.powers)
    terms = []
    for row in powers:
        term = torch.ones((), dtype=torch.float64)
        for p, k in enumerate(row):
            for _ in range(int(k)): term = term * dx[p]       # (integer powers by products: exact derivatives at dx = 0 too)
        terms.append(term)
    derivatives = torch.as_tensor(np.asarray(engine.derivatives, dtype='f8'))
    return torch.tensordot(torch.stack(terms), derivatives, dims=([0], [0]))


def predict(x, engine):
    return taylor_predict(x, engine) if hasattr(engine, 'powers') else mlp_predict(x, engine)


class EmulatedJacobianOracle(EmulatedOracle):
    """``names``: the columns of the Fisher context (``Fisher.varied_params.names()``: the varied parameters, then the solved ones); nothing is solved here."""

    def __init__(self, like, pt, theory, in_params, model, names):
        super(EmulatedJacobianOracle, self).__init__(like, pt, theory, [], in_params, model)
        self.names = list(names)

    def flat(self, p):
        eng = self.pt.engines
        xin = torch.stack([torch.as_tensor(p[name], dtype=torch.float64) for name in self.in_params])
        pktable = predict(xin, eng['pktable']).reshape(3, -1, 19)
        sigma8 = predict(xin, eng['sigma8']).reshape(-1)[0]
        fsigma8 = predict(xin, eng['fsigma8']).reshape(-1)[0]
        params = {name: p.get(name, self.like.all_params[name].value) for name in VPARS}
        th = self.theory
        pars = velocileptors_pars(params, sigma8, fsigma8 / sigma8, self.model, th.snd, th.fsat, th.sigv)
        table = pktable @ monomials(pars, th.nd)
        power = table @ self.interp.T
        return self.wfull @ torch.ravel(power + self.snin[:, None]) - self.snout

    def flat_theta(self, theta):
        return self.flat({name: theta[i] for i, name in enumerate(self.names)})

    def jacobian(self, row):
        """(flat [n], J [n, P]) at one centre."""
        theta = torch.tensor(np.asarray(row, dtype='f8'))
        J = torch.autograd.functional.jacobian(self.flat_theta, theta)
        return self.flat_theta(theta).detach().numpy(), J.numpy()

    def fisher(self, row):
        """(offset_ref, gradient_ref [P], hessian_ref [P, P], J [n, P]) at one centre."""
        flat, J = self.jacobian(row)
        diff, precision = flat - self.data.numpy(), self.precision.numpy()
        return -0.5 * diff @ precision @ diff, -J.T @ precision @ diff, -J.T @ precision @ J, J
