"""Cases for the MLP trainer (csrc/dl_mlp.hip: ``dl_mlp_*``, ``_lib.MLPTrainer``) beyond the one network of tests/test_gpu_mlp_train.py: networks, row counts and
batches chosen for the branches of the strided fp64 MFMA GEMM (16 x 16 tiles, a 16-step K loop, then 4-step tails), of the loss kernel (a grid-stride pass beyond
1024 x 256 elements) and of the trainer (1 to 16 layers).  No device library here: tests/test_mlp_cases.py proves on the CPU that the table reaches what it says and
that the compared numbers notice a lost tail, tests/test_gpu_mlp_shapes.py runs the kernels on it.

Tolerances: the project's for this kernel (tests/test_gpu_mlp_train.py).  tests/test_mlp_cases.py measures, per case, the distance of the float64 oracle from the same
oracle in ``np.longdouble`` (the floor) and asserts that 8 x floor fits under them, so no case needs a bound of its own."""
import collections

import numpy as np

from oracle import np_oracle as orc

TILE, KSTEP, KLOOP = 16, 4, 16        # csrc/dl_mlp.hip: one wavefront per 16 x 16 tile; v_mfma_f64_16x16x4; four k-steps per loop iteration
LOSS_SINGLE_PASS = 1024 * 256         # dl_mlp_backprop: at most 1024 workgroups of 256 threads; beyond, the loss kernel strides
MAX_LAYERS = 16

# the project's tolerances for this kernel (tests/test_gpu_mlp_train.py)
TOL = dict(loss_rtol=1e-13, grad_rtol=1e-11, grad_atol=1e-14, forward_rtol=1e-12, forward_atol=1e-13, adam_loss_rtol=1e-9, weight_rtol=1e-8, weight_atol=1e-10)

# name -> widths, rows, batch, steps, activation, seed; ``reaches``: what the case is there for (asserted by tests/test_mlp_cases.py::test_table_reaches_its_branches)
# batch: one that does not divide the rows where the rows allow it and the case is not about exact tiles; batch == rows (one chunk) in ``exact16`` and ``stride``
CASES = collections.OrderedDict([
    ('one', dict(widths=[1, 1], rows=1, batch=1, steps=25, activation='silu', seed=11, reaches=('single_layer', 'all_one', 'k_lt_4'))),
    ('exact16', dict(widths=[16, 16, 16, 16], rows=16, batch=16, steps=25, activation='tanh', seed=12, reaches=('no_tail', 'one_tile'))),
    ('exact_multi', dict(widths=[16, 32, 48, 64], rows=64, batch=48, steps=25, activation='relu', seed=13, reaches=('no_tail', 'several_tiles'))),
    ('under', dict(widths=[3, 15, 2, 1], rows=15, batch=7, steps=25, activation='silu', seed=14, reaches=('m_lt_16', 'n_lt_16', 'k_lt_4', 'k_tail', 'width_one'))),
    ('over_silu', dict(widths=[4, 17, 31, 35], rows=17, batch=5, steps=25, activation='silu', seed=15, reaches=('k_tail', 'k_mod16_1_15_3', 'one_past_tile'))),
    ('over_tanh', dict(widths=[4, 17, 31, 35], rows=17, batch=5, steps=25, activation='tanh', seed=15, reaches=('k_tail', 'k_mod16_1_15_3', 'one_past_tile'))),
    ('over_relu', dict(widths=[4, 17, 31, 35], rows=17, batch=5, steps=25, activation='relu', seed=15, reaches=('k_tail', 'k_mod16_1_15_3', 'one_past_tile'))),
    ('deep', dict(widths=[2] + [5] * 15 + [3], rows=9, batch=4, steps=25, activation='tanh', seed=16, reaches=('layer_limit', 'm_lt_16', 'n_lt_16'))),
    ('single_row', dict(widths=[5, 33, 17, 70], rows=1, batch=1, steps=25, activation='relu', seed=23, reaches=('rows_one',))),     # (a seed at which no K tail falls on a dead relu unit of the one row)
    ('stride_silu', dict(widths=[7, 24, 1021], rows=257, batch=257, steps=8, activation='silu', seed=19, reaches=('loss_second_pass',))),
    ('stride_tanh', dict(widths=[7, 24, 1021], rows=257, batch=257, steps=8, activation='tanh', seed=19, reaches=('loss_second_pass',))),
    ('stride_relu', dict(widths=[7, 24, 1021], rows=257, batch=257, steps=8, activation='relu', seed=19, reaches=('loss_second_pass',))),     # (seed: the last hidden unit, the one a lost K tail drops, is alive under relu)
])

LR = 3e-3


def names():
    return list(CASES)


def build(name):
    """(layers, x, y) of the case: weights ~ N(0, 1 / fan_in), biases ~ 0.05 N(0, 1), x uniform in [0, 1), y ~ N(0, 1) -- as in tests/test_gpu_mlp_train.py."""
    case = CASES[name]
    rng = np.random.RandomState(case['seed'])
    widths = case['widths']
    layers = [(rng.standard_normal((a, b)) / a**0.5, 0.05 * rng.standard_normal(b)) for a, b in zip(widths[:-1], widths[1:])]
    x, y = rng.uniform(0., 1., (case['rows'], widths[0])), rng.standard_normal((case['rows'], widths[-1]))
    return layers, x, y


def products(widths, rows):
    """(kind, layer, M, N, K) of every GEMM ``dl_mlp_backprop`` launches on ``rows`` rows: forward z_l = a_{l-1} W_l, dW_l = a_{l-1}^T delta_l, and for l > 0
    delta_{l-1} = delta_l W_l^T."""
    out = []
    for il, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        out.append(('forward', il, rows, b, a))
        out.append(('dw', il, a, b, rows))
        if il > 0: out.append(('delta', il, rows, a, b))
    return out


def flatten(grads):
    """List of (kernel, bias) -> the flat layout of ``dl_mlp``: kernel then bias, layer after layer."""
    return np.concatenate([np.concatenate([np.ravel(k), np.ravel(b)]) for k, b in grads])


def forward(layers, x, activation):
    a = x
    for il, (kernel, bias) in enumerate(layers):
        a = a.dot(kernel) + bias
        if il < len(layers) - 1: a = orc._mlp_act(a, activation)
    return a


def preactivations(layers, x, activation):
    zs, a = [], x
    for il, (kernel, bias) in enumerate(layers):
        z = a.dot(kernel) + bias
        zs.append(z)
        a = orc._mlp_act(z, activation) if il < len(layers) - 1 else z
    return zs


def loss_and_grad_variant(layers, x, y, activation, drop=None, loss_limit=None):
    """``orc.mlp_loss_and_grad`` with a planted error: ``drop = (kind, layer)`` loses the last ``K % 4`` (or, without tail, the last one) terms of that product, as a
    GEMM whose K tail is wrong would; ``loss_limit`` ignores the elements of the output beyond that flat index, as a loss kernel without its second pass would.
    With neither, the same numbers as the oracle's (asserted by tests/test_mlp_cases.py)."""
    def dot(kind, il, A, B):
        K = A.shape[1]
        if drop is not None and (kind, il) == tuple(drop):
            K -= (K % KSTEP) or 1
        return A[:, :K].dot(B[:K])

    zs, acts, a = [], [x], x
    for il, (kernel, bias) in enumerate(layers):
        z = dot('forward', il, a, kernel) + bias
        zs.append(z)
        a = orc._mlp_act(z, activation) if il < len(layers) - 1 else z
        acts.append(a)
    diff = a - y
    if loss_limit is not None:
        diff = diff.copy()
        diff.ravel()[loss_limit:] = 0.
    loss = np.sum(diff**2) / diff.size if loss_limit is not None else np.mean(diff**2)
    delta = 2. * diff / diff.size
    grads = [None] * len(layers)
    for il in range(len(layers) - 1, -1, -1):
        grads[il] = (dot('dw', il, acts[il].T, delta), delta.sum(axis=0))
        if il > 0: delta = dot('delta', il, delta, layers[il][0].T) * orc._mlp_act_prime(zs[il - 1], activation)
    return loss, grads


def as_longdouble(layers, x, y):
    return [(kernel.astype(np.longdouble), bias.astype(np.longdouble)) for kernel, bias in layers], x.astype(np.longdouble), y.astype(np.longdouble)


def staged(layers, x, y, batch, stages, activation):
    """The oracle's Adam in stages [(nsteps, lr), ...] as ``emulators.fit_mlp`` trains: moments, step count and chunk rotation carried across; (layers, losses, step)."""
    state, losses = {}, []
    for nsteps, lr in stages:
        layers, loss, state = orc.mlp_adam(layers, x, y, batch=batch, nsteps=nsteps, lr=lr, activation=activation, state=state)
        losses.append(loss)
    return layers, np.concatenate(losses), state['step']


# ---- edge inputs of tests/test_gpu_mlp_shapes.py (their soundness is asserted on the CPU by tests/test_mlp_cases.py) ----
SATURATION = 745.                      # exp(745) overflows, exp(-745) is the smallest subnormal


def saturation_case(activation):
    """[1, 19, 6] on 33 rows: the first layer maps x in [0, 1] onto pre-activations that span exactly [-745, 745] in its first unit (narrower, shifted spans in the
    others, so that the moderate range is sampled too)."""
    rng = np.random.RandomState(21)
    H, n_out, rows = 19, 6, 33
    scale = np.linspace(1., 0.02, H)
    kernel0, bias0 = (2. * SATURATION * scale)[None, :], -SATURATION * scale
    layers = [(kernel0, bias0), (rng.standard_normal((H, n_out)) / H**0.5, 0.05 * rng.standard_normal(n_out))]
    x, y = np.linspace(0., 1., rows)[:, None], rng.standard_normal((rows, n_out))
    return layers, x, y, activation


def relu_zero_case():
    """[4, 9, 6, 3] on 11 rows, relu, the second hidden layer with zero kernel and zero bias: its pre-activation is exactly 0, where the derivative of relu is 0
    (oracle: ``z > 0``), so that no gradient reaches the layers before and its own kernel."""
    rng = np.random.RandomState(22)
    widths, rows = [4, 9, 6, 3], 11
    layers = [(rng.standard_normal((a, b)) / a**0.5, 0.05 * rng.standard_normal(b)) for a, b in zip(widths[:-1], widths[1:])]
    layers[1] = (np.zeros_like(layers[1][0]), np.zeros_like(layers[1][1]))
    x, y = rng.uniform(0., 1., (rows, widths[0])), rng.standard_normal((rows, widths[-1]))
    return layers, x, y, 'relu'
