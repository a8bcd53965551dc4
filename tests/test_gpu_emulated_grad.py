"""GPU (-m gpu): analytic log-posterior gradient of MLP-emulated full-shape likelihoods with analytically solved parameters (csrc/dl_emu_grad.h) against the torch
autograd restatement of the NumPy oracle chain (tests/emu_grad_oracle.py); its plumbing, its scope and the samplers that consume it."""
import numpy as np
import pytest

from bench_configs import make_cfg3_full
from emulator_utils import CFG3_PARAMS, EMU_PARAMS
from emu_grad_oracle import EmulatedOracle
from test_gpu_emulator import make_mlp_likelihood

pytestmark = pytest.mark.gpu


def _theta(like, n, seed):
    rng = np.random.RandomState(seed)
    return np.column_stack([np.clip(param.ref.sample(size=n, random_state=rng), *param.prior.limits) for param in like.varied_params])


def _device_grad(like, theta):
    import torch
    ctx = like._get_context()
    t = torch.as_tensor(theta, device='cuda:{:d}'.format(ctx.device)).contiguous()
    out = ctx.eval_logposterior_grad(t)
    assert out is not None
    values = torch.empty(theta.shape[0], dtype=torch.float64, device=t.device)
    ctx.eval_logposterior(t, values)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), values.cpu().numpy()


def _check_rows(oracle, theta, lp, grad, lpe, rows):
    for i in rows:
        assert abs(lp[i] - lpe[i]) <= 1e-12 * max(1., abs(lpe[i])), (i, lp[i], lpe[i])
        value, ref = oracle.value_and_grad(theta[i])
        assert abs(lp[i] - value) <= 1e-9 * max(1., abs(value)), (i, lp[i], value)
        tol = 1e-9 * max(1., np.abs(ref).max())
        assert np.abs(grad[i] - ref).max() <= tol, (i, grad[i], ref)


@pytest.mark.parametrize('marg', [True, False])
def test_cfg3_full_gradient_4096(marg):
    g, like, pt, theory, solved = make_cfg3_full(marg=marg)
    theta = _theta(like, 4096, 3)
    lp, grad, lpe = _device_grad(like, theta)
    oracle = EmulatedOracle(like, pt, theory, solved, CFG3_PARAMS, 'rept')
    _check_rows(oracle, theta, lp, grad, lpe, (0, 15, 16, 100, 255, 256, 4095))


@pytest.mark.parametrize('hidden,activation,marg', [((8,), 'silu', True), ((24, 40), 'tanh', True), ((100,), 'relu', False), ((128, 128, 128, 128, 128), 'silu', True),
                                                    ((16, 16, 16, 16, 16, 16, 16), 'tanh', False), ((64, 32), 'relu', True), ((5, 7, 3), 'silu', False)])
def test_mlp_architectures_gradient(hidden, activation, marg):
    g, like, pt, theory, solved = make_mlp_likelihood(marg=marg, seed=5, hidden=hidden, activation=activation)
    theta = _theta(like, 257, 6)
    lp, grad, lpe = _device_grad(like, theta)
    oracle = EmulatedOracle(like, pt, theory, solved, EMU_PARAMS, 'lpt')
    _check_rows(oracle, theta, lp, grad, lpe, (0, 15, 16, 255, 256))


def test_best_marg_mix_gradient():
    kinds = {'alpha0p': '.best', 'alpha2p': '.marg', 'sn0p': '.marg', 'sn2p': '.best'}
    g, like, pt, theory, solved = make_mlp_likelihood(derived=kinds, seed=2)
    theta = _theta(like, 100, 8)
    lp, grad, lpe = _device_grad(like, theta)
    oracle = EmulatedOracle(like, pt, theory, solved, EMU_PARAMS, 'lpt', kinds=kinds)
    _check_rows(oracle, theta, lp, grad, lpe, (0, 17, 99))


def test_plumbing_batches_prior_and_repeatability():
    import torch
    g, like, pt, theory, solved = make_cfg3_full(marg=True)
    ctx = like._get_context()
    dev = 'cuda:{:d}'.format(ctx.device)
    theta = _theta(like, 5000, 4)
    names = like.varied_params.names()
    theta[7, names.index('qpar')] = 1.5            # outside its uniform prior
    t = torch.as_tensor(theta, device=dev).contiguous()
    status = torch.empty(5000, dtype=torch.int32, device=dev)
    lp, grad = ctx.eval_logposterior_grad(t, status=status)
    lp, grad, status = lp.cpu().numpy(), grad.cpu().numpy(), status.cpu().numpy()
    values, st = torch.empty(5000, dtype=torch.float64, device=dev), torch.empty(5000, dtype=torch.int32, device=dev)
    ctx.eval_logposterior(t, values, st)
    assert (status == st.cpu().numpy()).all() and status[7] != 0 and (np.delete(status, 7) == 0).all()
    assert lp[7] == -np.inf and (grad[7] == 0.).all()
    ok = status == 0
    assert np.all(np.abs(lp[ok] - values.cpu().numpy()[ok]) <= 1e-12 * np.maximum(1., np.abs(lp[ok])))
    lp2, grad2 = ctx.eval_logposterior_grad(t)
    assert np.array_equal(lp2.cpu().numpy(), lp) and np.array_equal(grad2.cpu().numpy(), grad)
    for B in (0, 1, 17):
        out = ctx.eval_logposterior_grad(t[:B].contiguous())
        assert out is not None and out[0].shape == (B,)
        if B:   # (the kernels and the split of the gradient GEMM depend on the batch size: equal to rounding)
            assert np.allclose(out[0].cpu().numpy(), lp[:B], rtol=1e-12, atol=0.)
            assert np.all(np.abs(out[1].cpu().numpy() - grad[:B]) <= 1e-10 * np.maximum(1., np.abs(grad[:B]).max(axis=1, keepdims=True)))


def test_parameter_reaching_no_theory_gets_prior_gradient_only():
    """sn4p varied with a Gaussian prior while the emulated tables of its monomial are zero: its gradient is the prior's, exactly."""
    import torch
    g, like, pt, theory, solved = make_mlp_likelihood(marg=True, seed=5)
    table = pt.engines['pktable']
    yl = np.array(table.ylimits, dtype='f8').reshape(3, -1, 19, 2)
    yl[:, :, 18, :] = 0.                                    # sn4 monomial: no table, the parameter reaches no theory
    table.ylimits = yl.reshape(-1, 2)
    theory.init.params['sn4p'].update(fixed=False, prior={'dist': 'norm', 'loc': 0.1, 'scale': 2.}, ref={'limits': [-0.5, 0.5]})
    names = like.varied_params.names()
    assert 'sn4p' in names
    i = names.index('sn4p')
    theta = _theta(like, 40, 9)
    ctx = like._get_context()
    out = ctx.eval_logposterior_grad(torch.as_tensor(theta, device='cuda:{:d}'.format(ctx.device)).contiguous())
    assert out is not None
    lp, grad = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.isfinite(lp).all()
    assert np.allclose(grad[:, i], -(theta[:, i] - 0.1) / 4., rtol=1e-13, atol=1e-15)


def test_out_of_scope_returns_none():
    import torch
    from bench_configs import make_cfg3_stacked
    from test_host_api import make_cfg3
    cases = [make_cfg3_stacked(marg=True, hidden=(32, 32), nk=30, seed=4)[0], make_cfg3()[1]]
    g, like, pt, theory, solved = make_mlp_likelihood(marg=True, seed=3)
    theory.init.params['b2p'].update(prior={'dist': 'cauchy', 'loc': 0., 'scale': 2.})    # general prior
    cases.append(like)
    from test_gpu_variants import build
    cases.append(build(template='shapefit', transform='cubic', covariance='diag', ells=(0, 2))[0])   # observable transform
    for like in cases:
        ctx = like._get_context()
        theta = _theta(like, 4, 1)
        t = torch.as_tensor(theta, device='cuda:{:d}'.format(ctx.device)).contiguous()
        assert ctx.eval_logposterior_grad(t) is None


def _short_chain(kind, gradient):
    from desilike_amd.samplers import HMCSampler, NUTSSampler
    g, like, pt, theory, solved = make_cfg3_full(marg=True)
    if kind == 'hmc':
        s = HMCSampler(like, chains=64, adaptation=False, step_size=0.02, num_integration_steps=10, gradient=gradient, seed=7)
    else:
        s = NUTSSampler(like, chains=64, adaptation=False, step_size=0.01, gradient=gradient, seed=7)
    s.run(max_iterations=120, check_every=120)
    x = np.concatenate([np.column_stack([c[n] for n in s.varied_params.names()])[20:] for c in s.chains])
    return x, float(np.mean(s.acceptance_rate)), s   # (NUTS: the mean acceptance statistic of its transitions, from the record's info)


@pytest.mark.parametrize('kind', ['hmc', 'nuts'])
def test_samplers_analytic_on_cfg3_full(kind):
    xa, acc_a, sa = _short_chain(kind, 'analytic')
    xf, acc_f, sf = _short_chain(kind, 'finite')
    assert np.isfinite(xa).all()
    if kind == 'hmc': assert abs(acc_a - acc_f) <= 0.05, (acc_a, acc_f)
    else:
        # NUTS integrates trajectories of up to 2^10 steps: the error of the central differences (Parameter.delta steps) does not shrink with the step size and holds
        # its acceptance statistic near 0.92 (0.92 at step sizes 0.02 and 0.01), while the exact gradient's rises towards 1 (0.97, 0.99).  A biased analytic
        # gradient would pull it down instead: it may not fall below the finite one's, and at this short step it must be near 1.
        assert acc_a >= acc_f - 0.05 and acc_a >= 0.97, (acc_a, acc_f)
    # chain means within 3 Monte-Carlo standard errors (64 chains: the chains are independent)
    ma, mf = xa.mean(axis=0), xf.mean(axis=0)
    se = np.sqrt(xa.var(axis=0) / 64 + xf.var(axis=0) / 64)
    assert np.all(np.abs(ma - mf) <= 3. * se + 1e-12), (ma, mf, se)
