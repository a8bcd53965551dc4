"""GPU (-m gpu): the MLP trainer (csrc/dl_mlp.hip, ``_lib.MLPTrainer``) on the cases of tests/mlp_cases.py against the oracle (``orc.mlp_loss_and_grad``,
``orc.mlp_adam``): forward, loss and gradient, Adam steps at every shape class of the strided MFMA GEMM and of the loss kernel, then the trainer's state (staged
training as ``emulators.fit_mlp`` does it, workspace growth, ``return_loss=False``, ``nsteps=0``, a non-default stream), saturated and exactly-zero pre-activations,
and the argument errors.  Tolerances: the project's for this kernel (``mlp_cases.TOL``); tests/test_mlp_cases.py shows on the CPU that 8 x the float64 oracle's
distance from ``np.longdouble`` fits under them at every case, and that they notice a lost K tail or a lost pass of the loss kernel.
Measured on an MI355X over the 12 cases: loss <= 1.6e-15 relative, gradient <= 2.6e-3 of its bound, forward <= 6e-16, Adam losses <= 1.6e-15 relative, weights <= 1.3e-15."""
import numpy as np
import pytest

import mlp_cases as mc
from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name):
    """Oracle numbers of the case, computed once and shared: loss, flat gradient, forward, Adam layers and losses."""
    if name not in _ref:
        case = mc.CASES[name]
        layers, x, y = mc.build(name)
        loss, grads = orc.mlp_loss_and_grad(layers, x, y, case['activation'])
        adam_layers, adam_losses = orc.mlp_adam(layers, x, y, batch=case['batch'], nsteps=case['steps'], lr=mc.LR, activation=case['activation'])
        _ref[name] = dict(loss=loss, grad=mc.flatten(grads), forward=mc.forward(layers, x, case['activation']), adam_layers=adam_layers, adam_losses=adam_losses)
        for value in _ref[name].values():
            if isinstance(value, np.ndarray): value.setflags(write=False)
    return _ref[name]


def on_device(*arrays):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda:0').contiguous() for a in arrays]


def check_loss_grad(loss, grad, ref_loss, ref_flat):
    tol = mc.TOL
    print('loss rel', abs(loss - ref_loss) / abs(ref_loss), 'grad max excess', (np.abs(grad - ref_flat) / (tol['grad_atol'] * np.abs(ref_flat).max() + tol['grad_rtol'] * np.abs(ref_flat))).max())
    assert abs(loss - ref_loss) <= tol['loss_rtol'] * abs(ref_loss)
    assert np.allclose(grad, ref_flat, rtol=tol['grad_rtol'], atol=tol['grad_atol'] * np.abs(ref_flat).max())


def check_weights(got_layers, ref_layers):
    tol = mc.TOL
    print('weights max abs', max(max(np.abs(k - rk).max(), np.abs(b - rb).max()) for (k, b), (rk, rb) in zip(got_layers, ref_layers)))
    for (kernel, bias), (rk, rb) in zip(got_layers, ref_layers):
        assert kernel.shape == rk.shape and bias.shape == rb.shape
        assert np.allclose(kernel, rk, rtol=tol['weight_rtol'], atol=tol['weight_atol']) and np.allclose(bias, rb, rtol=tol['weight_rtol'], atol=tol['weight_atol'])


def same_layers(a, b):
    return all(np.array_equal(ka, kb) and np.array_equal(ba, bb) for (ka, ba), (kb, bb) in zip(a, b))


@pytest.mark.parametrize('name', mc.names())
def test_forward_loss_gradient_and_adam_vs_oracle(name):
    from desilike_amd._lib import MLPTrainer
    case, tol = mc.CASES[name], mc.TOL
    layers, x, y = mc.build(name)
    ref = reference(name)
    xt, yt = on_device(x, y)
    trainer = MLPTrainer(layers, activation=case['activation'], device=0)
    assert trainer.info('n_layers') == len(layers) and trainer.info('n_in') == case['widths'][0] and trainer.info('n_out') == case['widths'][-1]
    assert trainer.n_weights == ref['grad'].size and trainer.info('step') == 0
    out = trainer.forward(xt).cpu().numpy()
    print('forward max abs', np.abs(out - ref['forward']).max())
    assert out.shape == ref['forward'].shape and np.allclose(out, ref['forward'], rtol=tol['forward_rtol'], atol=tol['forward_atol'])
    loss, grad = trainer.loss_and_grad(xt, yt)
    check_loss_grad(loss, grad, ref['loss'], ref['grad'])
    assert same_layers(trainer.layers(), layers) and trainer.info('step') == 0          # neither call touches the weights
    losses = trainer.train(xt, yt, batch=case['batch'], nsteps=case['steps'], lr=mc.LR)
    print('adam losses rel', np.abs(losses / ref['adam_losses'] - 1.).max())
    assert losses.shape == ref['adam_losses'].shape and np.allclose(losses, ref['adam_losses'], rtol=tol['adam_loss_rtol'], atol=0.)
    check_weights(trainer.layers(), ref['adam_layers'])
    assert trainer.info('step') == case['steps']
    trainer.close()


def test_staged_training_like_fit_mlp():
    """Three ``train`` calls with decaying lr (``emulators.fit_mlp``: Adam step and chunk rotation carried across calls) against the oracle's staged run; with equal lr,
    calls of n1 and n2 steps are the one call of n1 + n2, bit for bit."""
    from desilike_amd._lib import MLPTrainer
    name = 'over_silu'
    case = mc.CASES[name]
    layers, x, y = mc.build(name)
    xt, yt = on_device(x, y)
    stages = [(7, 3e-3), (5, 1e-3), (9, 3e-4)]          # 21 steps on 3 chunks: every call starts on another chunk
    trainer = MLPTrainer(layers, activation=case['activation'], device=0)
    losses = np.concatenate([trainer.train(xt, yt, batch=case['batch'], nsteps=nsteps, lr=lr) for nsteps, lr in stages])
    ref_layers, ref_losses, ref_step = mc.staged(layers, x, y, case['batch'], stages, case['activation'])
    assert trainer.info('step') == ref_step == 21
    print('staged losses rel', np.abs(losses / ref_losses - 1.).max())
    assert np.allclose(losses, ref_losses, rtol=mc.TOL['adam_loss_rtol'], atol=0.)
    check_weights(trainer.layers(), ref_layers)
    # the schedule matters: the single-lr run of as many steps is somewhere else
    single = orc.mlp_adam(layers, x, y, batch=case['batch'], nsteps=21, lr=3e-3, activation=case['activation'])[1]
    assert not np.allclose(single[12:], ref_losses[12:], rtol=1e-6, atol=0.)
    trainer.close()
    one, two = MLPTrainer(layers, activation=case['activation'], device=0), MLPTrainer(layers, activation=case['activation'], device=0)
    whole = one.train(xt, yt, batch=case['batch'], nsteps=11, lr=mc.LR)
    parts = np.concatenate([two.train(xt, yt, batch=case['batch'], nsteps=4, lr=mc.LR), two.train(xt, yt, batch=case['batch'], nsteps=7, lr=mc.LR)])
    assert np.array_equal(whole, parts) and same_layers(one.layers(), two.layers()) and one.info('step') == two.info('step') == 11
    one.close(); two.close()


def test_workspace_growth_leaves_no_trace():
    """forward on 5 rows, loss_and_grad on 40, forward on 300, then train with batch 7 on one trainer (``dl_mlp_reserve`` grows twice, then serves a smaller batch from
    the larger workspace) = a fresh trainer that only trains, bit for bit; the intermediate results match the oracle."""
    from desilike_amd._lib import MLPTrainer
    rng = np.random.RandomState(31)
    widths, act, tol = [4, 17, 31, 35], 'tanh', mc.TOL
    layers = [(rng.standard_normal((a, b)) / a**0.5, 0.05 * rng.standard_normal(b)) for a, b in zip(widths[:-1], widths[1:])]
    x, y = rng.uniform(0., 1., (300, widths[0])), rng.standard_normal((300, widths[-1]))
    xt, yt = on_device(x, y)
    used = MLPTrainer(layers, activation=act, device=0)
    assert np.allclose(used.forward(xt[:5].contiguous()).cpu().numpy(), mc.forward(layers, x[:5], act), rtol=tol['forward_rtol'], atol=tol['forward_atol'])
    loss, grad = used.loss_and_grad(xt[:40].contiguous(), yt[:40].contiguous())
    ref_loss, ref_grads = orc.mlp_loss_and_grad(layers, x[:40], y[:40], act)
    check_loss_grad(loss, grad, ref_loss, mc.flatten(ref_grads))
    assert np.allclose(used.forward(xt).cpu().numpy(), mc.forward(layers, x, act), rtol=tol['forward_rtol'], atol=tol['forward_atol'])
    fresh = MLPTrainer(layers, activation=act, device=0)
    kwargs = dict(batch=7, nsteps=12, lr=mc.LR)
    assert np.array_equal(used.train(xt[:40].contiguous(), yt[:40].contiguous(), **kwargs), fresh.train(xt[:40].contiguous(), yt[:40].contiguous(), **kwargs))
    assert same_layers(used.layers(), fresh.layers())
    ref_layers, ref_losses = orc.mlp_adam(layers, x[:40], y[:40], activation=act, **kwargs)
    check_weights(used.layers(), ref_layers)
    # and a forward on the full 300 rows after training: the trained weights, the large workspace
    assert np.allclose(used.forward(xt).cpu().numpy(), mc.forward(used.layers(), x, act), rtol=tol['forward_rtol'], atol=tol['forward_atol'])
    used.close(); fresh.close()


def test_return_loss_false_and_zero_steps():
    from desilike_amd._lib import MLPTrainer
    name = 'under'
    case = mc.CASES[name]
    layers, x, y = mc.build(name)
    xt, yt = on_device(x, y)
    kwargs = dict(batch=case['batch'], lr=mc.LR)
    loud, quiet = MLPTrainer(layers, activation=case['activation'], device=0), MLPTrainer(layers, activation=case['activation'], device=0)
    assert quiet.train(xt, yt, nsteps=9, return_loss=False, **kwargs) is None
    assert loud.train(xt, yt, nsteps=9, **kwargs).shape == (9,)
    assert same_layers(loud.layers(), quiet.layers()) and quiet.info('step') == 9
    before = loud.layers()
    for return_loss in (True, False):
        empty = loud.train(xt, yt, nsteps=0, return_loss=return_loss, **kwargs)
        assert (empty.shape == (0,) and empty.dtype == np.float64) if return_loss else empty is None
        assert loud.info('step') == 9 and same_layers(loud.layers(), before)
    # the run goes on as if the empty calls had not happened
    assert np.array_equal(loud.train(xt, yt, nsteps=3, **kwargs), quiet.train(xt, yt, nsteps=3, **kwargs)) and same_layers(loud.layers(), quiet.layers())
    loud.close(); quiet.close()


def test_non_default_stream_gives_the_same_bits():
    import torch
    from desilike_amd._lib import MLPTrainer
    name = 'over_tanh'
    case = mc.CASES[name]
    layers, x, y = mc.build(name)
    xt, yt = on_device(x, y)
    base = MLPTrainer(layers, activation=case['activation'], device=0)
    out0 = base.forward(xt).cpu().numpy()
    loss0, grad0 = base.loss_and_grad(xt, yt)
    losses0 = base.train(xt, yt, batch=case['batch'], nsteps=10, lr=mc.LR)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    other = MLPTrainer(layers, activation=case['activation'], device=0)
    # once with the stream passed explicitly, once as torch's current stream (the default of every call)
    out1 = other.forward(xt, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(out1.cpu().numpy(), out0)
    with torch.cuda.stream(side):
        loss1, grad1 = other.loss_and_grad(xt, yt)
        losses1 = other.train(xt, yt, batch=case['batch'], nsteps=10, lr=mc.LR)
        layers1 = other.layers()
    side.synchronize()
    assert loss1 == loss0 and np.array_equal(grad1, grad0) and np.array_equal(losses1, losses0) and same_layers(layers1, base.layers())
    base.close(); other.close()


@pytest.mark.parametrize('activation', ['silu', 'tanh'])
def test_saturated_preactivations_stay_finite(activation):
    """Hidden pre-activations spanning [-745, 745]: exp overflows on one side and is subnormal on the other; forward, loss and gradient are finite and the oracle's."""
    from desilike_amd._lib import MLPTrainer
    layers, x, y, act = mc.saturation_case(activation)
    with np.errstate(over='ignore'):
        ref_loss, ref_grads = orc.mlp_loss_and_grad(layers, x, y, act)
        ref_out = mc.forward(layers, x, act)
    xt, yt = on_device(x, y)
    trainer = MLPTrainer(layers, activation=act, device=0)
    out = trainer.forward(xt).cpu().numpy()
    loss, grad = trainer.loss_and_grad(xt, yt)
    assert np.isfinite(out).all() and np.isfinite(loss) and np.isfinite(grad).all()
    assert np.allclose(out, ref_out, rtol=mc.TOL['forward_rtol'], atol=mc.TOL['forward_atol'])
    check_loss_grad(loss, grad, ref_loss, mc.flatten(ref_grads))
    # a few Adam steps from there stay finite too
    losses = trainer.train(xt, yt, batch=11, nsteps=5, lr=mc.LR)
    assert np.isfinite(losses).all() and all(np.isfinite(k).all() and np.isfinite(b).all() for k, b in trainer.layers())
    trainer.close()


def test_relu_derivative_at_zero_is_zero():
    """A hidden layer with zero kernel and bias: pre-activation exactly 0, derivative 0 as in the oracle (``z > 0``): no gradient before it, exactly."""
    from desilike_amd._lib import MLPTrainer
    layers, x, y, act = mc.relu_zero_case()
    ref_loss, ref_grads = orc.mlp_loss_and_grad(layers, x, y, act)
    ref_flat = mc.flatten(ref_grads)
    xt, yt = on_device(x, y)
    trainer = MLPTrainer(layers, activation=act, device=0)
    loss, grad = trainer.loss_and_grad(xt, yt)
    check_loss_grad(loss, grad, ref_loss, ref_flat)
    n_zero = ref_flat.size - layers[2][1].size          # everything but the last bias
    assert not ref_flat[:n_zero].any() and not grad[:n_zero].any() and grad[n_zero:].all()
    trainer.close()


def test_argument_errors_are_errors():
    import torch
    from desilike_amd._lib import MLPTrainer, LibraryError
    name = 'under'
    case = mc.CASES[name]
    layers, x, y = mc.build(name)
    xt, yt = on_device(x, y)
    trainer = MLPTrainer(layers, activation=case['activation'], device=0)
    for batch in (case['rows'] + 1, 0):
        with pytest.raises(LibraryError, match='dl_mlp_train: need 1 <= batch <= n_samples and n_steps >= 0'):
            trainer.train(xt, yt, batch=batch, nsteps=2)
    with pytest.raises(LibraryError, match='dl_mlp_loss_and_grad: invalid argument'):
        trainer.loss_and_grad(xt[:0].contiguous(), yt[:0].contiguous())
    empty = trainer.forward(xt[:0].contiguous())
    assert tuple(empty.shape) == (0, case['widths'][-1]) and empty.dtype == torch.float64
    # the trainer is as before: nothing ran
    assert trainer.info('step') == 0 and same_layers(trainer.layers(), layers)
    trainer.close()
    with pytest.raises(LibraryError, match='dl_mlp_create: layer widths must be positive'):
        MLPTrainer([(np.zeros((3, 0)), np.zeros(0)), (np.zeros((0, 2)), np.zeros(2))], activation='silu', device=0)
    rng = np.random.RandomState(1)
    seventeen = [(rng.standard_normal((2, 2)), np.zeros(2)) for _ in range(17)]
    with pytest.raises(LibraryError, match='dl_mlp_create: 1 to 16 layers'):
        MLPTrainer(seventeen, activation='silu', device=0)
    MLPTrainer(seventeen[:16], activation='silu', device=0).close()
