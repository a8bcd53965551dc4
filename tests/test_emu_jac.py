"""CPU: the per-point arithmetic of the emulated analytic Jacobian (csrc/dl_emu_jac.h) built for the host (tests/csrc/emulate_emu_jac.cpp) against torch autograd: the
forward mode of the 19 monomials, MLP and Taylor engines with their tangents, and the transpose identity with the reverse mode tests/test_emu_grad.py pins.
Bounds: those of tests/test_emu_grad.py (1e-13 of max(1, largest reference entry); values 1e-14)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_emu_grad import _lib as _grad_lib, _p, _torch_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ACTS = {'silu': 0, 'relu': 1, 'tanh': 2}


def _lib():
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_emu_jac.so')
    src = os.path.join(HERE, 'csrc', 'emulate_emu_jac.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_emu_jac.h', 'dl_emu_grad.h', 'dl_fullshape.h']]
    if not os.path.isfile(so) or any(os.path.getmtime(dep) > os.path.getmtime(so) for dep in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, src])
    lib = ctypes.CDLL(so)
    vp, d, i = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    lib.emu_ej_mono_jvp.argtypes = [i, d, d, d, d, vp, d, d, vp]
    lib.emu_ej_mlp.argtypes = [i, i, vp, i, i, vp, vp, vp, d, d, vp, i, vp, vp, vp]
    lib.emu_ej_taylor.argtypes = [i, i, vp, vp, vp, vp, i, vp, vp, vp]
    return lib


CONSTS = dict(nd=3e-4, snd=0.8, fsat=0.1, sigv=5.)


def _mono_case(mono_mode, it):
    rng = np.random.RandomState(10 * mono_mode + it)
    return rng.uniform(0.5, 1.5, 11), rng.uniform(0.7, 0.9), rng.uniform(0.4, 0.5)


def _device_jacobian(lib, mono_mode, v, s8, fs8):
    J = np.zeros((13, 19))
    lib.emu_ej_mono_jvp(mono_mode, CONSTS['nd'], CONSTS['snd'], CONSTS['fsat'], CONSTS['sigv'], _p(v), s8, fs8, _p(J))
    return J


@pytest.mark.parametrize('mono_mode', [1, 2, 3, 4])
def test_mono_jacobian_vs_autograd(mono_mode):
    import torch
    lib = _lib()
    slots = np.full(11, -1, dtype='i4')
    for it in range(5):
        v, s8, fs8 = _mono_case(mono_mode, it)

        def row0(inputs):
            return _torch_rows(list(inputs[:11]), inputs[11], inputs[12], mono_mode, CONSTS['nd'], CONSTS['snd'], CONSTS['fsat'], CONSTS['sigv'], slots)[0]

        ref = torch.autograd.functional.jacobian(row0, torch.tensor(np.concatenate([v, [s8, fs8]]))).numpy().T      # [13, 19]
        J = _device_jacobian(lib, mono_mode, v, s8, fs8)
        err = np.abs(J - ref).max() / max(1., np.abs(ref).max())
        print('mono_mode {:d}: {:.2e}'.format(mono_mode, err))
        assert err <= 1e-13, (mono_mode, it, err)
        if mono_mode in (3, 4): assert (J[11:] == 0.).all()          # the direct basis does not see sigma8 / fsigma8: exact zeros


@pytest.mark.parametrize('mono_mode', [1, 2, 3, 4])
def test_transpose_identity_with_the_reverse_mode(mono_mode):
    """y^T (J v) = v^T dl_eg_mono_vjp(y): the forward mode is the transpose of the reverse mode tests/test_emu_grad.py checks."""
    lib, glib = _lib(), _grad_lib()
    slots = np.full(11, -1, dtype='i4')
    for it in range(5):
        v, s8, fs8 = _mono_case(mono_mode, it)
        rng = np.random.RandomState(100 + it)
        y, t = rng.standard_normal(19), rng.standard_normal(13)
        J = _device_jacobian(lib, mono_mode, v, s8, fs8)              # [13, 19]: d mono_m / d input_k
        g = np.zeros(13)
        glib.emu_eg_mono_vjp(mono_mode, CONSTS['nd'], CONSTS['snd'], CONSTS['fsat'], CONSTS['sigv'], _p(slots), 0, _p(v), s8, fs8, _p(np.ascontiguousarray(y[None, :])), _p(g))
        forward, reverse = y @ (J.T @ t), t @ g
        scale = max(1., np.abs(J.T * y[:, None] * t[None, :]).max())
        assert abs(forward - reverse) <= 1e-13 * scale, (mono_mode, forward, reverse)


def _mlp(rng, n_x, widths):
    layers, last = [], n_x
    for width in widths:
        layers.append((rng.standard_normal((last, width)) / last**0.5, 0.1 * rng.standard_normal(width)))
        last = width
    return layers


def _torch_mlp(x, xlimits, layers, activation, table, ylimits):
    import torch
    from emu_grad_oracle import _act
    xl = torch.as_tensor(xlimits)
    a = (x - xl[:, 0]) / (xl[:, 1] - xl[:, 0])
    for ilayer, (kernel, bias) in enumerate(layers):
        a = a @ torch.as_tensor(kernel) + torch.as_tensor(bias)
        if table or ilayer < len(layers) - 1: a = _act(a, activation)
    return a if table else a * (ylimits[1] - ylimits[0]) + ylimits[0]


@pytest.mark.parametrize('activation', ['silu', 'relu', 'tanh'])
@pytest.mark.parametrize('width', [5, 64, 65])
def test_mlp_tangents_vs_autograd(activation, width):
    """Table engine (every layer activated, the hidden units are the basis) and scalar engine (linear last layer, y-scaler), inputs 0 and 2 of 3 varied; every
    instantiation (4, 8, 16 tangents) gives the same numbers."""
    import torch
    lib = _lib()
    rng = np.random.RandomState(width + ACTS[activation])
    xlimits = np.array([[0.9, 1.1], [0.9, 1.1], [-0.1, 0.1]])
    xlo, xinv = np.ascontiguousarray(xlimits[:, 0]), np.ascontiguousarray(1. / (xlimits[:, 1] - xlimits[:, 0]))
    varied = np.array([1, 0, 1], dtype='i4')
    ylimits = (0.7, 0.9)
    for table in (1, 0):
        layers = _mlp(rng, 3, [width, width] if table else [width, width, 1])
        widths = np.array([3] + [kernel.shape[1] for kernel, bias in layers], dtype='i4')
        weights = np.concatenate([np.concatenate([kernel.ravel(), bias]) for kernel, bias in layers])
        nout = int(widths[-1])
        for it in range(3):
            x = np.array([rng.uniform(*lim) for lim in xlimits])
            f = lambda xt: _torch_mlp(xt, xlimits, layers, activation, table, ylimits)
            ref_value = f(torch.tensor(x)).numpy()
            ref = torch.autograd.functional.jacobian(f, torch.tensor(x)).numpy().T[[0, 2]]        # [2, nout]
            outs = []
            for nt in (4, 8, 16):
                value, tangent = np.zeros(nout), np.zeros((2, nout))
                assert lib.emu_ej_mlp(3, len(layers), _p(widths), ACTS[activation], table, _p(xlo), _p(xinv), _p(weights), ylimits[0], ylimits[1] - ylimits[0], _p(varied), nt,
                                      _p(x), _p(value), _p(tangent)) == 0
                outs.append((value, tangent))
            assert all(np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1]) for o in outs[1:])
            value, tangent = outs[0]
            assert np.allclose(value, ref_value, rtol=1e-14, atol=1e-14 * max(1., np.abs(ref_value).max()))
            err = np.abs(tangent - ref).max() / max(1., np.abs(ref).max())
            print('{} width {:d} table {:d}: {:.2e}'.format(activation, width, table, err))
            assert err <= 1e-13, (activation, width, table, err)


def test_relu_derivative_at_zero_is_zero():
    """One unit, pre-activation exactly 0 (zero kernel, zero bias): relu'(0) = 0, jax's convention."""
    lib = _lib()
    widths = np.array([1, 1], dtype='i4')
    weights, xlo, xinv, varied, x = np.zeros(2), np.zeros(1), np.ones(1), np.ones(1, dtype='i4'), np.array([0.3])
    weights[0] = 1.
    value, tangent = np.ones(1), np.ones((1, 1))
    assert lib.emu_ej_mlp(1, 1, _p(widths), 1, 1, _p(xlo), _p(xinv), _p(weights), 0., 1., _p(varied), 4, _p(np.zeros(1)), _p(value), _p(tangent)) == 0
    assert value[0] == 0. and tangent[0, 0] == 0.
    assert lib.emu_ej_mlp(1, 1, _p(widths), 1, 1, _p(xlo), _p(xinv), _p(weights), 0., 1., _p(varied), 4, _p(x), _p(value), _p(tangent)) == 0
    assert value[0] == 0.3 and tangent[0, 0] == 1.


def test_taylor_tangents_on_the_cfg3_state():
    """The engines of emulator_utils.taylor_state: the table engine's basis (the monomials themselves) and the two scalar engines, all three inputs varied."""
    import torch
    from golden_utils import load_golden
    from emulator_utils import taylor_state
    from emu_jac_oracle import taylor_predict
    from desilike_amd.emulators import TaylorEmulatorEngine
    lib = _lib()
    state = taylor_state(load_golden('cfg3_velocileptors_table'))
    rng = np.random.RandomState(3)
    varied = np.ones(3, dtype='i4')
    for name in ('pktable', 'sigma8', 'fsigma8'):
        center, powers = np.asarray(state[name]['center'], dtype='f8'), np.asarray(state[name]['powers'], dtype='f8')
        n_terms = len(powers)
        scalar = name != 'pktable'
        derivatives = np.asarray(state[name]['derivatives'], dtype='f8') if scalar else np.eye(n_terms)      # (the table engine's outputs are the monomials)
        engine = TaylorEmulatorEngine(center=center, powers=powers.astype('i4'), derivatives=derivatives)
        nout = 1 if scalar else n_terms
        for x in [center + rng.uniform(-0.05, 0.05, 3) for it in range(3)] + [center.copy()]:      # (the centre itself: 0^0 = 1 and the first-order terms' derivatives)
            f = lambda xt: taylor_predict(xt, engine).reshape(-1)
            ref_value, ref = f(torch.tensor(x)).numpy(), torch.autograd.functional.jacobian(f, torch.tensor(x)).numpy().T
            value, tangent = np.zeros(nout), np.zeros((3, nout))
            coef = np.ascontiguousarray(derivatives.ravel()) if scalar else None
            assert lib.emu_ej_taylor(3, n_terms, _p(center), _p(np.ascontiguousarray(powers)), _p(coef) if scalar else None, _p(varied), 4, _p(np.ascontiguousarray(x)), _p(value), _p(tangent)) == 0
            assert np.allclose(value, ref_value, rtol=1e-14, atol=1e-14)
            assert np.abs(tangent - ref).max() <= 1e-13 * max(1., np.abs(ref).max()), (name, tangent, ref)
