"""CPU: the cases of tests/mlp_cases.py (networks, rows and batches for the branches of csrc/dl_mlp.hip) -- that every case builds, that the oracle's gradient is the
derivative of its loss, that continuing the oracle's Adam from a state is the single run bit for bit, that the table reaches the GEMM / loss-kernel / layer-count
branches it names, that the project's tolerances leave room for 8 x the float64 oracle's own distance from ``np.longdouble``, and that the compared gradient notices a
lost K tail or a lost second pass of the loss kernel.  No device library."""
import numpy as np
import pytest

import mlp_cases as mc
from oracle import np_oracle as orc

_built, _ref = {}, {}


def built(name):
    if name not in _built: _built[name] = mc.build(name)
    return _built[name]


def reference(name):
    """float64 oracle of the case, computed once: loss, flat gradient."""
    if name not in _ref:
        layers, x, y = built(name)
        loss, grads = orc.mlp_loss_and_grad(layers, x, y, mc.CASES[name]['activation'])
        _ref[name] = (loss, mc.flatten(grads))
    return _ref[name]


def grad_tolerance(ref):
    """The element-wise bound the GPU test puts on the gradient."""
    return mc.TOL['grad_atol'] * np.abs(ref).max() + mc.TOL['grad_rtol'] * np.abs(ref)


@pytest.mark.parametrize('name', mc.names())
def test_case_builds(name):
    case = mc.CASES[name]
    layers, x, y = built(name)
    widths = case['widths']
    assert [k.shape for k, b in layers] == list(zip(widths[:-1], widths[1:])) and [b.shape for k, b in layers] == [(w,) for w in widths[1:]]
    assert x.shape == (case['rows'], widths[0]) and y.shape == (case['rows'], widths[-1])
    assert 1 <= len(layers) <= mc.MAX_LAYERS and 1 <= case['batch'] <= case['rows'] and 1 <= case['steps'] <= 25
    loss, flat = reference(name)
    assert np.isfinite(loss) and np.isfinite(flat).all() and loss > 0. and np.abs(flat).max() > 0.
    # the planted-error oracle without an error is the oracle
    vloss, vgrads = mc.loss_and_grad_variant(layers, x, y, case['activation'])
    assert vloss == loss and np.array_equal(mc.flatten(vgrads), flat)
    assert np.array_equal(mc.forward(layers, x, case['activation']), mc.preactivations(layers, x, case['activation'])[-1])


def test_batches_cover_ragged_and_single_chunk():
    ragged = [name for name, case in mc.CASES.items() if case['rows'] % case['batch'] != 0]
    single = [name for name, case in mc.CASES.items() if case['rows'] == case['batch'] and case['rows'] > 1]
    rotating = [name for name, case in mc.CASES.items() if 1 < case['rows'] // case['batch'] < case['steps']]
    assert len(ragged) >= 5 and len(single) >= 2 and len(rotating) >= 4
    for name in ('over', 'stride'):
        assert {mc.CASES['{}_{}'.format(name, act)]['activation'] for act in ('silu', 'tanh', 'relu')} == {'silu', 'tanh', 'relu'}
    assert {case['activation'] for name, case in mc.CASES.items() if not name.startswith(('over', 'stride'))} == {'silu', 'tanh', 'relu'}


@pytest.mark.parametrize('name', mc.names())
def test_oracle_gradient_vs_finite_differences(name):
    """Central differences of the oracle's loss on the weight of largest gradient and a few drawn ones.  Step 1e-6 on a loss of O(1): rounding ~ 1e-16 / 1e-6, truncation
    ~ 1e-12 f''': bound 1e-8 (1 + |g|)."""
    case = mc.CASES[name]
    layers, x, y = built(name)
    loss, flat = reference(name)
    rng = np.random.RandomState(5)
    picks = sorted(set([int(np.abs(flat).argmax())] + list(rng.randint(0, flat.size, 5))))
    h = 1e-6

    def loss_at(index, shift):
        moved, off = [], 0
        for kernel, bias in layers:
            kernel, bias = kernel.copy(), bias.copy()
            for arr in (kernel, bias):
                if off <= index < off + arr.size: arr.ravel()[index - off] += shift
                off += arr.size
            moved.append((kernel, bias))
        return orc.mlp_loss_and_grad(moved, x, y, case['activation'])[0]

    for index in picks:
        fd = (loss_at(index, h) - loss_at(index, -h)) / (2. * h)
        assert abs(fd - flat[index]) <= 1e-8 * (1. + abs(flat[index])), (name, index, fd, flat[index])


@pytest.mark.parametrize('name', ['over_silu', 'under', 'single_row'])
def test_oracle_adam_in_stages_is_the_single_run(name):
    """``state``: k stages with equal lr = one run, bit for bit (moments, step count and the chunk rotation carry over); the default call is untouched by it."""
    case = mc.CASES[name]
    layers, x, y = built(name)
    kwargs = dict(batch=case['batch'], lr=mc.LR, activation=case['activation'])
    ref_layers, ref_losses = orc.mlp_adam(layers, x, y, nsteps=13, **kwargs)
    for split in [(13,), (1, 12), (4, 0, 2, 7), (5, 5, 3)]:
        got_layers, got_losses, step = mc.staged(layers, x, y, case['batch'], [(n, mc.LR) for n in split], case['activation'])
        assert step == 13 and np.array_equal(got_losses, ref_losses)
        assert all(np.array_equal(gk, rk) and np.array_equal(gb, rb) for (gk, gb), (rk, rb) in zip(got_layers, ref_layers))
    # a different lr in a later stage leaves the earlier losses alone and changes the later ones
    got_layers, got_losses, step = mc.staged(layers, x, y, case['batch'], [(5, mc.LR), (8, 0.1 * mc.LR)], case['activation'])
    assert np.array_equal(got_losses[:6], ref_losses[:6]) and not np.array_equal(got_losses[6:], ref_losses[6:])
    # the input layers and an input state are not modified
    l1, _, state = orc.mlp_adam(layers, x, y, nsteps=3, state={}, **kwargs)
    snapshot = [[m.copy() for m in moment] for moment in state['moments']]
    orc.mlp_adam(l1, x, y, nsteps=2, state=state, **kwargs)
    assert state['step'] == 3 and all(np.array_equal(a, b) for ma, mb in zip(state['moments'], snapshot) for a, b in zip(ma, mb))


def test_table_reaches_its_branches():
    """(M, N, K) of the three products per layer, recomputed, against the classes each case is there for."""
    seen = set()
    for name, case in mc.CASES.items():
        prods = mc.products(case['widths'], case['rows'])
        Ms, Ns, Ks = ([p[i] for p in prods] for i in (2, 3, 4))
        reaches, n_layers = set(case['reaches']), len(case['widths']) - 1
        n_loss = case['rows'] * case['widths'][-1]
        have = set()
        if n_layers == 1: have.add('single_layer')
        if n_layers == mc.MAX_LAYERS: have.add('layer_limit')
        if all(v == 1 for v in Ms + Ns + Ks): have.add('all_one')
        if any(K < mc.KSTEP for K in Ks): have.add('k_lt_4')
        if all(K % mc.KLOOP == 0 for K in Ks): have.add('no_tail')
        if any(K % mc.KSTEP != 0 for K in Ks): have.add('k_tail')
        if any(M < mc.TILE for M in Ms): have.add('m_lt_16')
        if any(N < mc.TILE for N in Ns): have.add('n_lt_16')
        if 1 in case['widths'][1:-1] or (case['widths'][-1] == 1 and n_layers > 1): have.add('width_one')
        if all(v == mc.TILE for v in Ms + Ns + Ks): have.add('one_tile')
        if all(v % mc.TILE == 0 for v in Ms + Ns + Ks) and max(Ms) * max(Ns) > 4 * mc.TILE**2: have.add('several_tiles')      # more than the 4 tiles of one workgroup
        if {K % mc.KLOOP for K in Ks} >= {1, 15, 3}: have.add('k_mod16_1_15_3')
        if any(M == mc.TILE + 1 for M in Ms) and any(N == mc.TILE + 1 for N in Ns) and any(K == mc.TILE + 1 for K in Ks): have.add('one_past_tile')
        if case['rows'] == 1 and n_layers >= 3: have.add('rows_one')
        if n_loss > mc.LOSS_SINGLE_PASS and case['batch'] * case['widths'][-1] > mc.LOSS_SINGLE_PASS: have.add('loss_second_pass')       # in loss_and_grad and in train
        assert reaches <= have, (name, reaches - have)
        seen |= reaches
        # what the existing single network already covers must not be all a case has: every product of ``under`` has K of 1, 2, 3 or 15
        if name == 'under': assert set(Ks) == {1, 2, 3, 15}
        if name.startswith('stride'): assert n_loss == 262397
    assert seen == {'single_layer', 'all_one', 'k_lt_4', 'no_tail', 'one_tile', 'several_tiles', 'm_lt_16', 'n_lt_16', 'k_tail', 'width_one', 'k_mod16_1_15_3', 'one_past_tile',
                    'layer_limit', 'rows_one', 'loss_second_pass'}


@pytest.mark.parametrize('name', mc.names())
def test_tolerances_leave_room_for_the_oracle_floor(name):
    """The float64 oracle against itself in ``np.longdouble``: 8 x that distance (for the other summation order of the MFMA) must fit under the project's tolerances,
    element by element, for loss, gradient, forward and the Adam run -- else the case would need a bound of its own, written next to it."""
    case = mc.CASES[name]
    layers, x, y = built(name)
    act, tol = case['activation'], mc.TOL
    loss, flat = reference(name)
    ll, lx, ly = mc.as_longdouble(layers, x, y)
    hloss, hgrads = orc.mlp_loss_and_grad(ll, lx, ly, act)
    hflat = mc.flatten(hgrads)
    assert hflat.dtype == np.longdouble
    assert 8. * abs(loss - hloss) <= tol['loss_rtol'] * abs(hloss), abs(loss - hloss) / abs(hloss)
    floor = np.abs(flat - hflat)
    assert (8. * floor <= tol['grad_atol'] * np.abs(hflat).max() + tol['grad_rtol'] * np.abs(hflat)).all(), floor.max() / np.abs(hflat).max()
    out, hout = mc.forward(layers, x, act), mc.forward(ll, lx, act)
    assert (8. * np.abs(out - hout) <= tol['forward_atol'] + tol['forward_rtol'] * np.abs(hout)).all(), np.abs(out - hout).max()
    steps = case['steps'] if case['rows'] * case['widths'][-1] <= mc.LOSS_SINGLE_PASS else 3       # (longdouble products of the large case are slow: 3 of its 8 steps)
    (rl, rlosses), (hl, hlosses) = (orc.mlp_adam(*args, batch=case['batch'], nsteps=steps, lr=mc.LR, activation=act) for args in ((layers, x, y), (ll, lx, ly)))
    assert (8. * np.abs(rlosses - hlosses) <= tol['adam_loss_rtol'] * np.abs(hlosses)).all(), np.abs(rlosses / hlosses - 1.).max()
    for (rk, rb), (hk, hb) in zip(rl, hl):
        for r, h in ((rk, hk), (rb, hb)):
            assert (8. * np.abs(r - h) <= tol['weight_atol'] + tol['weight_rtol'] * np.abs(h)).all(), np.abs(r - h).max()


@pytest.mark.parametrize('name', mc.names())
def test_comparison_notices_a_lost_tail(name):
    """Every product of the case with its last K % 4 (or last one) terms lost moves some element of the gradient by at least 1e3 x the bound the GPU test puts on it:
    the inputs are not degenerate in a way that would hide a wrong K tail."""
    case = mc.CASES[name]
    layers, x, y = built(name)
    loss, flat = reference(name)
    bound = grad_tolerance(flat)
    for kind, il, M, N, K in mc.products(case['widths'], case['rows']):
        vloss, vgrads = mc.loss_and_grad_variant(layers, x, y, case['activation'], drop=(kind, il))
        moved = np.abs(mc.flatten(vgrads) - flat)
        assert (moved >= 1e3 * bound).any(), (name, kind, il, (moved / bound).max())


@pytest.mark.parametrize('name', [name for name in mc.names() if 'loss_second_pass' in mc.CASES[name]['reaches']])
def test_comparison_notices_a_lost_second_pass(name):
    """The loss kernel without its grid-stride pass (elements past 1024 x 256 skipped) moves loss and gradient by far more than their bounds."""
    case = mc.CASES[name]
    layers, x, y = built(name)
    loss, flat = reference(name)
    vloss, vgrads = mc.loss_and_grad_variant(layers, x, y, case['activation'], loss_limit=mc.LOSS_SINGLE_PASS)
    moved = np.abs(mc.flatten(vgrads) - flat)
    assert (moved >= 1e3 * grad_tolerance(flat)).any() and abs(vloss - loss) >= 1e3 * mc.TOL['loss_rtol'] * abs(loss)
    # and nothing before the limit moves: the last layer's bias gradient of the columns the skipped elements do not touch
    n_out = case['widths'][-1]
    untouched = np.arange(n_out) < (mc.LOSS_SINGLE_PASS % n_out)       # the last, partial row starts at column (limit % n_out); rows after it are lost entirely
    assert case['rows'] * n_out - mc.LOSS_SINGLE_PASS < n_out and np.array_equal(mc.flatten(vgrads)[-n_out:][untouched], flat[-n_out:][untouched])


def test_edge_inputs_are_what_they_say():
    """Saturation: the first hidden pre-activation spans exactly [-745, 745], exp overflows there and the oracle stays finite.  relu at zero: the zeroed layer's
    pre-activation is exactly 0 and the oracle sends no gradient through it."""
    for activation in ('silu', 'tanh'):
        layers, x, y, act = mc.saturation_case(activation)
        with np.errstate(over='ignore'):
            z = mc.preactivations(layers, x, act)[0]
            assert z.min() == -mc.SATURATION and z.max() == mc.SATURATION and np.isinf(np.exp(mc.SATURATION)) and np.exp(-mc.SATURATION) > 0.
            assert ((np.abs(z) > 1.) & (np.abs(z) < 30.)).sum() > 50          # the unsaturated range is sampled as well
            loss, grads = orc.mlp_loss_and_grad(layers, x, y, act)
            out = mc.forward(layers, x, act)
        flat = mc.flatten(grads)
        assert np.isfinite(loss) and np.isfinite(flat).all() and np.isfinite(out).all() and np.abs(flat[:19]).max() > 0.
    layers, x, y, act = mc.relu_zero_case()
    zs = mc.preactivations(layers, x, act)
    assert np.array_equal(zs[1], np.zeros_like(zs[1])) and (zs[0] > 0.).any()
    loss, grads = orc.mlp_loss_and_grad(layers, x, y, act)
    assert all(not g.any() for pair in grads[:2] for g in pair) and not grads[2][0].any() and grads[2][1].any()
