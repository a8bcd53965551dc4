"""CPU: the analytic gradient of emulated full-shape likelihoods -- the torch restatement of the NumPy oracle (tests/emu_grad_oracle.py) against that oracle and against
Richardson-extrapolated central differences of it, and the host build of the per-point arithmetic of csrc/dl_emu_grad.h (tests/csrc/emulate_emu_grad.cpp) against
torch autograd."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_emu_grad.so')
    src = os.path.join(HERE, 'csrc', 'emulate_emu_grad.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_emu_grad.h', 'dl_fullshape.h']]
    if not os.path.isfile(so) or any(os.path.getmtime(dep) > os.path.getmtime(so) for dep in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, src])
    lib = ctypes.CDLL(so)
    common = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    lib.emu_eg_mono.argtypes = common + [ctypes.c_void_p]
    lib.emu_eg_mono_vjp.argtypes = common + [ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_eg_marg_adjoint.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 7
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _torch_rows(v, s8, fs8, mono_mode, nd, snd, fsat, sigv, slots):
    """Monomial rows as torch tensors: row 0 and, for each solved slot, d row0 / d v_c (the theory is linear in the solved inputs)."""
    import torch
    from emu_grad_oracle import velocileptors_pars, monomials
    physical, rept = mono_mode in (1, 2), mono_mode in (2, 4)
    names = ['b1p', 'b2p', 'bsp', 'b3p', 'alpha0p', 'alpha2p', 'alpha4p', 'alpha6', 'sn0p', 'sn2p', 'sn4p']
    if physical:
        pars = velocileptors_pars(dict(zip(names, v)), s8, fs8 / s8, 'rept' if rept else 'lpt', snd, fsat, sigv)
    else:
        pars = list(v)
        if rept:
            b1 = pars[0]
            pars[2] = pars[2] - (2 / 7) * (b1 - 1.)
            pars[3] = 3 * pars[3] + (b1 - 1.)
    row0 = monomials(pars, nd)
    rows = [row0]
    n_var = max(slots) + 1 if max(slots) >= 0 else 0
    drows = [None] * n_var
    for c in range(4, 11):
        if slots[c] < 0: continue
        d = []
        for m in range(19):
            gm = torch.autograd.grad(row0[m], v[c], create_graph=True, allow_unused=True)[0] if row0[m].requires_grad else None
            d.append(gm if gm is not None else torch.zeros((), dtype=torch.float64))
        drows[slots[c]] = torch.stack(d)
    return torch.stack(rows + drows)


@pytest.mark.parametrize('mono_mode', [1, 2, 3, 4])
def test_mono_vjp_vs_autograd(mono_mode):
    import torch
    lib = _lib()
    rng = np.random.RandomState(mono_mode)
    nd, snd, fsat, sigv = 3e-4, 0.8, 0.1, 5.
    slots = np.full(11, -1, dtype='i4')
    for slot, c in enumerate([4, 5, 6, 8, 9]): slots[c] = slot
    n_var = 5
    for it in range(5):
        v = rng.uniform(0.5, 1.5, 11)
        s8, fs8 = rng.uniform(0.7, 0.9), rng.uniform(0.4, 0.5)
        Q = rng.standard_normal((1 + n_var, 19))
        vt = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in v]
        s8t, fs8t = torch.tensor(s8, dtype=torch.float64, requires_grad=True), torch.tensor(fs8, dtype=torch.float64, requires_grad=True)
        rows = _torch_rows(vt, s8t, fs8t, mono_mode, nd, snd, fsat, sigv, slots)
        mono = np.zeros((1 + n_var, 19))
        lib.emu_eg_mono(mono_mode, nd, snd, fsat, sigv, _p(slots), n_var, _p(v), s8, fs8, _p(mono))
        assert np.allclose(mono, rows.detach().numpy(), rtol=1e-14, atol=1e-14 * np.abs(mono).max())
        J = (torch.as_tensor(Q) * rows).sum()
        ref = torch.autograd.grad(J, vt + [s8t, fs8t], allow_unused=True)
        ref = np.array([0. if r is None else float(r) for r in ref])
        g = np.zeros(13)
        lib.emu_eg_mono_vjp(mono_mode, nd, snd, fsat, sigv, _p(slots), n_var, _p(v), s8, fs8, _p(Q), _p(g))
        scale = max(1., np.abs(ref).max())
        assert np.abs(g - ref).max() <= 1e-13 * scale, (mono_mode, g, ref)


@pytest.mark.parametrize('kinds', [(1, 1, 1, 1, 1), (1, 0, 1, 0, 1), (0, 0, 0), (1,)])
def test_marg_adjoint_vs_autograd(kinds):
    """y_0 = -r*, y_s = -r* dx_s + sum_t Wc_st Tt_t (dl_emu_grad.h) are the gradients of the marginalised log-likelihood w.r.t. dt and the rows Tt_s."""
    import torch
    lib = _lib()
    rng = np.random.RandomState(len(kinds) + sum(kinds))
    ns, n = len(kinds), 40
    is_marg = np.array(kinds, dtype='i4')
    x0, loc = rng.uniform(-0.5, 0.5, ns), rng.uniform(-0.5, 0.5, ns)
    prec = np.where(rng.uniform(size=ns) < 0.3, 0., rng.uniform(0.1, 2., ns))
    dt = torch.tensor(rng.standard_normal(n), requires_grad=True)
    T = torch.tensor(rng.standard_normal((ns, n)), requires_grad=True)
    pt = torch.as_tensor(prec)
    A = T @ T.T + torch.diag(pt)
    dx = torch.linalg.solve(A, -(T @ dt) - torch.as_tensor((x0 - loc) * prec))
    r = dt + T.T @ dx
    J = -0.5 * r @ r - 0.5 * torch.sum(pt * (torch.as_tensor(x0) + dx - torch.as_tensor(loc))**2)
    m = np.flatnonzero(is_marg)
    if m.size: J = J - 0.5 * torch.linalg.slogdet(A[torch.as_tensor(m)][:, torch.as_tensor(m)])[1]
    gdt, gT = torch.autograd.grad(J, [dt, T])
    X = np.vstack([dt.detach().numpy(), T.detach().numpy()])
    G = np.ascontiguousarray(X @ X.T)
    dxc, Wc = np.zeros(ns), np.zeros((ns, ns))
    assert lib.emu_eg_marg_adjoint(ns, _p(G), _p(x0), _p(loc), _p(prec), _p(is_marg), _p(dxc), _p(Wc)) == 0
    assert np.allclose(dxc, dx.detach().numpy(), rtol=1e-13, atol=1e-13)
    Tn = X[1:]
    rs = X[0] + dxc @ Tn
    y0 = -rs
    ys = -rs[None, :] * dxc[:, None] + Wc @ Tn
    scale = max(1., np.abs(gT.numpy()).max(), np.abs(gdt.numpy()).max())
    assert np.abs(y0 - gdt.numpy()).max() <= 1e-13 * scale
    assert np.abs(ys - gT.numpy()).max() <= 1e-13 * scale


def _cfg(kind):
    import sys
    sys.path.insert(0, os.path.join(HERE, '..'))
    from emulator_utils import CFG3_PARAMS, EMU_PARAMS
    if kind == 'cfg3':
        from bench_configs import make_cfg3_full
        g, like, pt, theory, solved = make_cfg3_full(marg=True)
        return like, pt, theory, solved, CFG3_PARAMS, 'rept'
    from test_gpu_emulator import make_mlp_likelihood
    marg, activation = kind
    g, like, pt, theory, solved = make_mlp_likelihood(marg=marg, seed=5, hidden=(24, 40), activation=activation)
    return like, pt, theory, solved, EMU_PARAMS, 'lpt'


def _numpy_logposterior(like, pt, theory, solved, in_params, model, row):
    from oracle import np_oracle as orc
    from test_gpu_emulator import oracle_flat
    from bench_configs import cfg3_oracle_solution
    names = like.varied_params.names()
    if model == 'rept':
        sol = cfg3_oracle_solution(like, pt, theory, solved, row)
        value = sol['loglikelihood'] + sol.get('logprior_solved', 0.)
    else:
        nsol = len(solved)
        f0 = oracle_flat(like, pt, theory, row, names, {name: 0. for name in solved})
        if nsol:
            scales = np.array([like.all_params[name].prior.scale for name in solved])
            T = np.array([oracle_flat(like, pt, theory, row, names, {n2: float(n2 == name) for n2 in solved}) - f0 for name in solved])
            sol = orc.solve_marginalized(f0 - like.flatdata, T, like.precision, x0=np.zeros(nsol), prior_loc=np.zeros(nsol), prior_scale=scales, marg_mask=np.ones(nsol, dtype='?'))
            value = sol['loglikelihood'] + sol['logprior_solved']
        else:
            value = orc.gaussian_loglikelihood(f0, like.flatdata, like.precision)[0]
    for i, param in enumerate(like.varied_params):
        if param.prior.dist == 'norm': value += -0.5 * ((row[i] - param.prior.loc) / param.prior.scale)**2
    return value


@pytest.mark.parametrize('kind', ['cfg3', (True, 'silu'), (False, 'tanh'), (True, 'relu')])
def test_torch_oracle_vs_numpy_oracle(kind):
    from emu_grad_oracle import EmulatedOracle
    like, pt, theory, solved, in_params, model = _cfg(kind)
    like.initialize()
    oracle = EmulatedOracle(like, pt, theory, solved, in_params, model)
    rng = np.random.RandomState(2)
    row = np.array([np.clip(p.ref.sample(random_state=rng), *p.prior.limits) for p in like.varied_params])
    value, grad = oracle.value_and_grad(row)
    ref = _numpy_logposterior(like, pt, theory, solved, in_params, model, row)
    assert abs(value - ref) <= 1e-12 * max(1., abs(ref))
    # Richardson-extrapolated central differences of the NumPy oracle
    f = lambda x: _numpy_logposterior(like, pt, theory, solved, in_params, model, x)
    for i in range(len(row)):
        h = (1e-5 if kind[-1:] == ('relu',) else 1e-3) * max(1., abs(row[i]))   # (relu: a step that straddles no kink)
        def cd(step):
            e = np.zeros_like(row); e[i] = step
            return (f(row + e) - f(row - e)) / (2. * step)
        d1, d2 = cd(h), cd(h / 2.)
        rich = (4. * d2 - d1) / 3.
        assert abs(grad[i] - rich) <= 1e-6 * max(1., abs(grad[i])), (kind, i, grad[i], rich)
