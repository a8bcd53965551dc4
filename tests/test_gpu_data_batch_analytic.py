"""GPU (-m gpu): the exact derivatives against a data batch -- ``dl_eval_fisher_analytic_data`` and ``dl_eval_logposterior_grad_data`` (csrc/dl_data_batch.h:
dl_data_resid_kernel), through ``Context.eval_fisher_analytic_data`` / ``eval_logposterior_grad_data``, ``DataBatch.logposterior_grad`` and
``Fisher(method='analytic').evaluate(centers, data_index)``.

Reference of every value: the project's single-data path -- a context created from the same configuration with ``obs<i>.flatdata`` replaced by data vector m, evaluated
with ``dl_eval_fisher_analytic`` / ``dl_eval_logposterior_grad`` (the twins).  Shapes: those of tests/test_gpu_data_batch.py::test_fisher_data, 3 centres x 5 mocks of
``reference(name)``.  Tolerances: offset rtol 1e-10, atol 1e-9 and gradients 1e-8 of their largest entry (what test_fisher_data applies to the same comparison on the
finite route); log-posteriors 1e-10 max(1, |ref|) (the data batch's own); the Hessian does not depend on the data: the BITS of ``dl_eval_fisher_analytic`` of the same
centres on the batch context itself.  Central differences: the bound of tests/test_fisher.py:195."""
import functools

import numpy as np
import pytest

from data_batch_utils import get_case, reference
from test_gpu_data_batch import CASES, _context, _tol, _marg_likelihood, _marg_mocks

pytestmark = pytest.mark.gpu

NC, NM = 3, 5
NAN_INPUT = 3      # DL_STATUS_NAN_INPUT
SENTINEL = -777.
EMULATED = ('boundary_cfg3',)      # the configuration of CASES on the emulated feature path: the gradient entry point answers 2 there, whatever its twin does


def _t(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array), device=torch.device('cuda', 0))


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


def _rows(theta, nc=NC, nm=NM):
    """Row c nm + m: centre c against mock m (the layout of test_fisher_data)."""
    return np.ascontiguousarray(np.repeat(theta[:nc], nm, axis=0)), np.tile(np.arange(nm, dtype='i4'), nc)


@functools.lru_cache(maxsize=None)
def _scopes():
    """(names of CASES on which dl_eval_fisher_analytic answers, names on which the Kaiser branch of dl_eval_logposterior_grad answers), each context asked once."""
    fisher, grad = [], []
    for name in CASES:
        case, mocks, theta, _, _ = reference(name)
        ctx = _context(case)
        centers = _t(theta[:NC])
        if ctx.eval_fisher_analytic(centers) is not None: fisher.append(name)
        if name not in EMULATED and ctx.eval_logposterior_grad(centers) is not None: grad.append(name)
        ctx.close()
    return tuple(fisher), tuple(grad)


@functools.lru_cache(maxsize=None)
def _per_mock(name):
    """The twins on the NM per-mock contexts at centres theta[:NC], computed once: fisher (hessian, gradient, offset) [NM][...] where dl_eval_fisher_analytic answers,
    gradient (logposterior, grad, status) [NM][...] where dl_eval_logposterior_grad does; None otherwise."""
    import torch
    case, mocks, theta, _, _ = reference(name)
    centers = _t(theta[:NC])
    fisher, grad = [], []
    for m in range(NM):
        single = _context(case, mocks[m])
        out = single.eval_fisher_analytic(centers)
        fisher.append(None if out is None else _np(out))
        status = torch.full((NC,), -1, dtype=torch.int32, device=centers.device)
        out = single.eval_logposterior_grad(centers, status=status)
        grad.append(None if out is None else _np(out) + [status.cpu().numpy()])
        single.close()
    for block in fisher + grad:
        for array in block or []: array.setflags(write=False)
    return fisher, grad


def _check_fisher_rows(name, rows, centre_of, mock_of, gradient, offset, worst):
    fisher, _ = _per_mock(name)
    for row in rows:
        rh, rg, ro = fisher[mock_of[row]]
        c = centre_of[row]
        oerr = abs(offset[row] - ro[c])
        gerr = np.abs(gradient[row] - rg[c]).max() / np.abs(rg[c]).max()
        worst[:] = np.maximum(worst, [oerr / (1e-9 + 1e-10 * abs(ro[c])), gerr])
        assert oerr <= 1e-9 + 1e-10 * abs(ro[c]), (name, row, offset[row], ro[c])
        assert gerr <= 1e-8, (name, row, gerr)


# ---- 1. Fisher --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_fisher_analytic_data(name):
    """dl_eval_fisher_analytic_data against dl_eval_fisher_analytic on the per-mock contexts, 3 centres x 5 mocks; the Hessian: the bits of dl_eval_fisher_analytic of
    the same centres on the batch context itself.  Outside the twin's scope both answer None."""
    import torch
    in_scope = _scopes()[0]
    assert 'cfg2_shapefit_window' in in_scope and 'boundary_two_tracers' in in_scope, in_scope
    case, mocks, theta, _, _ = reference(name)
    centers, index = _rows(theta)
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    out = ctx.eval_fisher_analytic_data(_t(centers), _t(index))
    own = ctx.eval_fisher_analytic(_t(centers))
    if name not in in_scope:
        assert out is None and own is None
        ctx.close()
        return
    assert out is not None
    torch.cuda.synchronize()
    assert torch.equal(out[0], own[0])                  # the Hessian: bitwise, whatever the index
    hessian, gradient, offset = _np(out)
    assert np.isfinite(hessian).all() and np.isfinite(gradient).all() and np.isfinite(offset).all()
    worst = np.zeros(2)
    _check_fisher_rows(name, range(NC * NM), np.repeat(np.arange(NC), NM), index, gradient, offset, worst)
    print('{}: worst differences to dl_eval_fisher_analytic of the per-mock contexts: offset {:.2e} of its tolerance, gradient {:.2e} of its largest entry'.format(name, *worst))
    for c in range(NC):
        for m in range(1, NM):
            assert np.array_equal(hessian[c * NM + m], hessian[c * NM])
    again = ctx.eval_fisher_analytic_data(_t(centers), _t(index))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, again))      # two calls: the same bits
    ctx.close()


def _emulated_setup():
    """(make_context(flatdata or None), own flatdata [n], centres [NC, P]) of an emulated configuration inside dl_fisher_emu_in_scope: boundary_cfg3 when it is, else the
    MLP likelihood of tests/test_gpu_emu_fisher_analytic.py (make_mlp_likelihood(marg=False, seed=5, hidden=(8,)))."""
    from desilike_amd._lib import Context
    case = get_case('boundary_cfg3')
    ctx = _context(case)
    theta = case.points(NC)
    ok = ctx.info('fisher_analytic_pass') > 0 and ctx.eval_fisher_analytic(_t(theta)) is not None
    ctx.close()
    if ok:
        return 'boundary_cfg3', (lambda flatdata=None: _context(case, flatdata)), case.flatdata, theta
    from test_gpu_emulator import make_mlp_likelihood
    from test_gpu_emu_fisher_analytic import _fisher, _centres
    g, like, pt, theory, solved = make_mlp_likelihood(marg=False, seed=5, hidden=(8,))
    fisher = _fisher(like)
    theta = _centres(fisher, NC, 6)
    flatdata = np.concatenate(like._flatdata_list())

    def make_context(data=None):
        return Context(like._spec({}, like._flatdata_list() if data is None else [np.asarray(data)], like._precision_input), device=like.device)

    ctx = make_context()
    ok = ctx.info('fisher_analytic_pass') > 0 and ctx.eval_fisher_analytic(_t(theta)) is not None
    ctx.close()
    if not ok: pytest.fail('no emulated configuration inside the scope of the emulated branch of dl_eval_fisher_analytic: neither boundary_cfg3 nor the MLP likelihood')
    return 'mlp (8,)', make_context, flatdata, theta


def test_fisher_analytic_data_emulated():
    """The emulated branch (dl_emu_jac_rows_kernel starting its sum from the bias row of the centre's data vector): per-mock contexts, the bits of the Hessian, a bad
    index; and the gradient entry point answers 2 on an emulated context."""
    import torch
    tag, make_context, flatdata, theta = _emulated_setup()
    mocks = flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(5).standard_normal((NM, flatdata.size))
    centers, index = _rows(theta)
    ctx = make_context()
    assert ctx.info('fisher_analytic_pass') > 0      # the emulated branch
    ctx.set_data_batch(mocks)
    out = ctx.eval_fisher_analytic_data(_t(centers), _t(index))
    own = ctx.eval_fisher_analytic(_t(centers))
    assert out is not None and own is not None
    torch.cuda.synchronize()
    assert torch.equal(out[0], own[0])
    hessian, gradient, offset = _np(out)
    worst = np.zeros(2)
    for m in range(NM):
        single = make_context(mocks[m])
        rh, rg, ro = _np(single.eval_fisher_analytic(_t(theta[:NC])))
        single.close()
        for c in range(NC):
            row = c * NM + m
            oerr, gerr = abs(offset[row] - ro[c]), np.abs(gradient[row] - rg[c]).max() / np.abs(rg[c]).max()
            worst = np.maximum(worst, [oerr / (1e-9 + 1e-10 * abs(ro[c])), gerr])
            assert oerr <= 1e-9 + 1e-10 * abs(ro[c]), (m, c, offset[row], ro[c])
            assert gerr <= 1e-8, (m, c, gerr)
    print('{}: worst differences to the per-mock contexts: offset {:.2e} of its tolerance, gradient {:.2e} of its largest entry'.format(tag, *worst))
    # the context's own data vector as vector 0 of a batch: the existing call and the data call start the same sum from the same bias
    ctx.set_data_batch(np.vstack([flatdata, mocks[:1]]))
    zero = ctx.eval_fisher_analytic_data(_t(centers), _t(np.zeros(len(centers), dtype='i4')))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(zero, own))
    # an index outside the table: NaN offset and gradient for that centre, the bits of the clean call everywhere else
    ctx.set_data_batch(mocks)
    bad = index.copy(); bad[2] = NM
    keep = np.arange(NC * NM) != 2
    hessian2, gradient2, offset2 = _np(ctx.eval_fisher_analytic_data(_t(centers), _t(bad)))
    assert np.isnan(offset2[2]) and np.isnan(gradient2[2]).all() and np.array_equal(hessian2, hessian)
    assert np.array_equal(offset2[keep], offset[keep]) and np.array_equal(gradient2[keep], gradient[keep])
    assert ctx.eval_logposterior_grad_data(_t(centers), _t(index)) is None
    ctx.close()


# ---- 2. gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_logposterior_grad_data(name):
    """dl_eval_logposterior_grad_data against dl_eval_logposterior_grad of the per-mock contexts and against dl_eval_logposterior_data; two calls give the same bits.
    Outside the Kaiser branch of the twin it answers None."""
    import torch
    in_scope = _scopes()[1]
    assert 'cfg2_shapefit_window' in in_scope and 'boundary_two_tracers' in in_scope, in_scope
    case, mocks, theta, _, _ = reference(name)
    centers, index = _rows(theta)
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    status = torch.full((NC * NM,), -1, dtype=torch.int32, device='cuda:0')
    out = ctx.eval_logposterior_grad_data(_t(centers), _t(index), status=status)
    if name not in in_scope:
        assert out is None
        ctx.close()
        return
    assert out is not None
    logposterior, grad = _np(out)
    status = status.cpu().numpy()
    paired = ctx.eval_logposterior_data(_t(centers), index=_t(index)).cpu().numpy()
    assert (np.abs(logposterior - paired) <= _tol(paired)).all(), np.abs(logposterior - paired).max()
    _, per_mock = _per_mock(name)
    worst = np.zeros(2)
    for c in range(NC):
        for m in range(NM):
            row = c * NM + m
            rlp, rgrad, rstatus = per_mock[m]
            lerr, gerr = abs(logposterior[row] - rlp[c]) / _tol(rlp[c]), np.abs(grad[row] - rgrad[c]).max() / np.abs(rgrad[c]).max()
            worst = np.maximum(worst, [lerr, gerr])
            assert status[row] == rstatus[c] == 0
            assert lerr <= 1., (name, row, logposterior[row], rlp[c])
            assert gerr <= 1e-8, (name, row, gerr)
    print('{}: worst differences to dl_eval_logposterior_grad of the per-mock contexts: log-posterior {:.2e} of its tolerance, gradient {:.2e} of the row\'s largest component'.format(name, *worst))
    again = ctx.eval_logposterior_grad_data(_t(centers), _t(index))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    ctx.close()


def test_gradient_against_central_differences():
    """cfg2_shapefit_window: the gradient against central differences of dl_eval_logposterior_data with the parameters' own steps (``Parameter.delta`` of the cfg2
    likelihood, shortened at the prior bounds: the stencil of fisher.logposterior_value_and_grad), the bound of tests/test_fisher.py:195."""
    from bench_configs import make_cfg2
    case, mocks, theta, _, _ = reference('cfg2_shapefit_window')
    g, like = make_cfg2()
    like.initialize()
    delta = {param.name: param.delta for param in like.varied_params}
    names = [str(n) for n in case.g['names']]
    assert sorted(names) == sorted(delta)
    centers, index = _rows(theta)
    B, P = centers.shape
    lower, upper = np.empty((B, P)), np.empty((B, P))
    for ip, pname in enumerate(names):
        lower[:, ip] = np.clip(np.minimum(delta[pname][1], centers[:, ip] - case.priors[ip, 1]), 0., None)
        upper[:, ip] = np.clip(np.minimum(delta[pname][2], case.priors[ip, 2] - centers[:, ip]), 0., None)
    points = np.repeat(centers[:, None, :], 2 * P + 1, axis=1)
    column = np.arange(P)
    points[:, 1 + 2 * column, column] -= lower
    points[:, 2 + 2 * column, column] += upper
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    logpost = ctx.eval_logposterior_data_host(points.reshape(-1, P), index=np.repeat(index, 2 * P + 1))[0].reshape(B, 2 * P + 1)
    finite = (logpost[:, 2::2] - logpost[:, 1::2]) / (lower + upper)
    logposterior, grad = _np(ctx.eval_logposterior_grad_data(_t(centers), _t(index)))
    ctx.close()
    assert np.isfinite(finite).all()
    print('cfg2: |analytic - central differences| up to {:.2e} of the largest gradient component'.format(np.abs(grad - finite).max() / np.abs(grad).max()))
    assert np.allclose(grad, finite, rtol=1e-3, atol=1e-5 * np.abs(grad).max())
    assert (np.abs(logposterior - logpost[:, 0]) <= _tol(logpost[:, 0])).all()


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
def test_single_row_and_single_vector():
    """B = 1 (one wavefront of the residual kernel) and M = 1, against the per-mock contexts."""
    import torch
    name = 'cfg2_shapefit_window'
    case, mocks, theta, _, _ = reference(name)
    fisher, grad = _per_mock(name)
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    worst = np.zeros(2)
    for M, m in [(NM, 3), (1, 0)]:
        if M == 1: assert ctx.set_data_batch(mocks[:1]) == 1
        centers, index = _t(theta[1:2]), _t(np.array([m], dtype='i4'))
        out = ctx.eval_fisher_analytic_data(centers, index)
        own = ctx.eval_fisher_analytic(centers)
        torch.cuda.synchronize()
        assert torch.equal(out[0], own[0])
        hessian, gradient, offset = _np(out)
        _check_fisher_rows(name, [0], [1], [m], gradient, offset, worst)
        status = torch.full((1,), -1, dtype=torch.int32, device='cuda:0')
        logposterior, g = _np(ctx.eval_logposterior_grad_data(centers, index, status=status))
        rlp, rgrad, rstatus = grad[m]
        assert int(status[0]) == rstatus[1] == 0 and abs(logposterior[0] - rlp[1]) <= _tol(rlp[1])
        assert np.abs(g[0] - rgrad[1]).max() <= 1e-8 * np.abs(rgrad[1]).max()
    # M = 1, several rows
    centers, index = _t(theta[:NC]), _t(np.zeros(NC, dtype='i4'))
    hessian, gradient, offset = _np(ctx.eval_fisher_analytic_data(centers, index))
    _check_fisher_rows(name, range(NC), np.arange(NC), np.zeros(NC, dtype='i4'), gradient, offset, worst)
    ctx.close()


def test_bad_index_rows():
    """B = 65 with an index of M at rows 2 and 64: NaN offset and gradient / NaN log-posterior with DL_STATUS_NAN_INPUT for those rows, the bits of the clean call for
    every other row, the Hessian of every row."""
    import torch
    case, mocks, theta, _, _ = reference('cfg2_shapefit_window')
    B = 65
    centers = _t(theta[:B])
    index = (np.arange(B) % NM).astype('i4')
    bad = index.copy(); bad[[2, 64]] = NM
    keep = np.ones(B, dtype='?'); keep[[2, 64]] = False
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    hessian, gradient, offset = _np(ctx.eval_fisher_analytic_data(centers, _t(index)))
    hessian2, gradient2, offset2 = _np(ctx.eval_fisher_analytic_data(centers, _t(bad)))
    assert np.isfinite(offset).all() and np.isfinite(gradient).all()
    assert np.isnan(offset2[~keep]).all() and np.isnan(gradient2[~keep]).all() and np.array_equal(hessian2, hessian)
    assert np.array_equal(offset2[keep], offset[keep]) and np.array_equal(gradient2[keep], gradient[keep])
    status, status2 = (torch.full((B,), -1, dtype=torch.int32, device='cuda:0') for i in range(2))
    logposterior, grad = _np(ctx.eval_logposterior_grad_data(centers, _t(index), status=status))
    logposterior2, grad2 = _np(ctx.eval_logposterior_grad_data(centers, _t(bad), status=status2))
    status, status2 = status.cpu().numpy(), status2.cpu().numpy()
    assert (status == 0).all() and np.isfinite(logposterior).all() and np.isfinite(grad).all()
    assert np.isnan(logposterior2[~keep]).all() and (status2[~keep] == NAN_INPUT).all()
    assert np.array_equal(logposterior2[keep], logposterior[keep]) and np.array_equal(grad2[keep], grad[keep]) and (status2[keep] == 0).all()
    # a negative index as well
    bad[2] = -1
    status3 = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    logposterior3, grad3 = _np(ctx.eval_logposterior_grad_data(centers, _t(bad), status=status3))
    offset3 = ctx.eval_fisher_analytic_data(centers, _t(bad))[2].cpu().numpy()
    assert np.isnan(logposterior3[2]) and int(status3[2]) == NAN_INPUT and np.isnan(offset3[2]) and np.array_equal(offset3[keep], offset[keep])
    ctx.close()


def test_rows_outside_the_priors_behave_as_in_the_twin():
    """A NaN row and a row above a prior bound through dl_eval_logposterior_grad_data (whose status and -inf come from dl_data_paired_kernel) against
    dl_eval_logposterior_grad of the per-mock contexts (dl_finalize_part): the same status, the same log-posterior and the same gradient row, bit for bit, on those rows;
    the other rows at the tolerances of test_logposterior_grad_data.  And the error messages of the shared implementations name the data entry points."""
    import ctypes
    import torch
    case, mocks, theta, _, _ = reference('cfg2_shapefit_window')
    B = 8
    rows = theta[:B].copy()
    rows[2, 2] = np.nan
    assert np.isfinite(case.priors[0, 2])
    rows[5, 0] = case.priors[0, 2] + 1.      # above the upper limit of parameter 0
    bad = np.zeros(B, dtype='?'); bad[[2, 5]] = True
    index = (np.arange(B) % NM).astype('i4')
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    logposterior, grad = _np(ctx.eval_logposterior_grad_data(_t(rows), _t(index), status=status))
    status = status.cpu().numpy()
    assert status[2] == NAN_INPUT and status[5] == 1 and (status[~bad] == 0).all()      # (1: DL_STATUS_OUT_OF_PRIOR)
    assert np.isneginf(logposterior[bad]).all()
    for m in range(NM):
        single = _context(case, mocks[m])
        rstatus = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
        rlp, rgrad = _np(single.eval_logposterior_grad(_t(rows), status=rstatus))
        rstatus = rstatus.cpu().numpy()
        single.close()
        for b in np.flatnonzero(index == m):
            assert status[b] == rstatus[b], (b, status[b], rstatus[b])
            if bad[b]:
                assert np.array_equal(logposterior[b], rlp[b]) and np.array_equal(grad[b], rgrad[b], equal_nan=True), (b, logposterior[b], rlp[b], grad[b], rgrad[b])
            else:
                assert abs(logposterior[b] - rlp[b]) <= _tol(rlp[b]) and np.abs(grad[b] - rgrad[b]).max() <= 1e-8 * np.abs(rgrad[b]).max(), b
    # a negative batch size: an error of the data entry points, under their own names
    centers = _t(rows)
    assert ctx._lib.dl_eval_fisher_analytic_data(ctx._handle, ctypes.c_void_p(centers.data_ptr()), -1, None, None, None, None, None) == 1
    assert b'dl_eval_fisher_analytic_data' in ctx._lib.dl_last_error(ctx._handle)
    assert ctx._lib.dl_eval_logposterior_grad_data(ctx._handle, ctypes.c_void_p(centers.data_ptr()), -1, None, None, None, None, None) == 1
    assert b'dl_eval_logposterior_grad_data' in ctx._lib.dl_last_error(ctx._handle)
    lp = torch.empty(B, dtype=torch.float64, device='cuda:0')
    assert ctx._lib.dl_eval_logposterior_grad_data(ctx._handle, ctypes.c_void_p(centers.data_ptr()), B, ctypes.c_void_p(_t(index).data_ptr()), ctypes.c_void_p(lp.data_ptr()), None, None, None) == 1
    assert b'dl_eval_logposterior_grad_data: invalid argument' in ctx._lib.dl_last_error(ctx._handle)
    ctx.close()


def test_two_passes():
    """boundary_two_tracers with B beyond one pass of each entry point (the pass rules of dl_eval_fisher_analytic and dl_eval_logposterior_grad): the rows of the second
    pass against the per-mock contexts, the Hessian against dl_eval_fisher_analytic of the same batch."""
    import torch
    name = 'boundary_two_tracers'
    case, mocks, theta, _, _ = reference(name)
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    P, K_pad, N_pad = theta.shape[1], ctx.info('K_pad'), ctx.info('N_pad')
    per_pass = max(64, min(2048, (16 << 20) // ((1 + P) * max(K_pad, N_pad))) // 64 * 64)      # centres per pass of dl_eval_fisher_analytic
    B = per_pass + 7
    assert B > per_pass
    centre_of, mock_of = np.arange(B) % NC, ((np.arange(B) // NC) % NM).astype('i4')
    centers, index = _t(theta[centre_of]), _t(mock_of)
    out = ctx.eval_fisher_analytic_data(centers, index)
    own = ctx.eval_fisher_analytic(centers)
    torch.cuda.synchronize()
    assert torch.equal(out[0], own[0])
    hessian, gradient, offset = _np(out)
    worst = np.zeros(2)
    _check_fisher_rows(name, list(range(4)) + list(range(per_pass - 2, B)), centre_of, mock_of, gradient, offset, worst)
    # the gradient: passes of 2048 points
    per_pass = 2048
    B = per_pass + 7
    assert B > per_pass
    centre_of, mock_of = np.arange(B) % NC, ((np.arange(B) // NC) % NM).astype('i4')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    logposterior, grad = _np(ctx.eval_logposterior_grad_data(_t(theta[centre_of]), _t(mock_of), status=status))
    assert (status.cpu().numpy() == 0).all()
    _, per_mock = _per_mock(name)
    for row in list(range(4)) + list(range(per_pass - 2, B)):
        rlp, rgrad, rstatus = per_mock[mock_of[row]]
        c = centre_of[row]
        assert abs(logposterior[row] - rlp[c]) <= _tol(rlp[c]), row
        assert np.abs(grad[row] - rgrad[c]).max() <= 1e-8 * np.abs(rgrad[c]).max(), row
    print('{}: two passes: worst offset {:.2e} of its tolerance, gradient {:.2e} of its largest entry'.format(name, *worst))
    ctx.close()


def test_refusals():
    """A context with solved parameters and a context without a data batch: return code 1 with a message; cfg4_bao_xi: return code 2 / None from both entry points with
    nothing launched -- the outputs keep the sentinel they were filled with."""
    import torch
    from desilike_amd import LibraryError
    from desilike_amd._lib import Context
    from test_gpu_boundary import load_fixture
    device = torch.device('cuda', 0)
    # solved parameters
    sctx = Context(load_fixture('two_tracers_marg')[1], device=0)
    assert sctx.n_solved > 0
    sctx.set_data_batch(np.ones((2, sctx.n_data)), solved=True)
    centers = torch.zeros((2, sctx.n_params), dtype=torch.float64, device=device)
    index = torch.zeros(2, dtype=torch.int32, device=device)
    with pytest.raises(LibraryError, match='solved'):
        sctx.eval_fisher_analytic_data(centers, index)
    with pytest.raises(LibraryError, match='solved'):
        sctx.eval_logposterior_grad_data(centers, index)
    sctx.close()
    # no data batch
    case, mocks, theta, _, _ = reference('cfg2_shapefit_window')
    ctx = _context(case)
    centers, index = _t(theta[:2]), torch.zeros(2, dtype=torch.int32, device=device)
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_fisher_analytic_data(centers, index)
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_logposterior_grad_data(centers, index)
    # a null index with B > 0
    ctx.set_data_batch(mocks[:2])
    import ctypes
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device=device)
    assert ctx._lib.dl_eval_fisher_analytic_data(ctx._handle, ctypes.c_void_p(centers.data_ptr()), 2, None, None, None, ctypes.c_void_p(out.data_ptr()), None) == 1
    assert b'null data index' in ctx._lib.dl_last_error(ctx._handle)
    grad = torch.full((2, theta.shape[1]), SENTINEL, dtype=torch.float64, device=device)
    assert ctx._lib.dl_eval_logposterior_grad_data(ctx._handle, ctypes.c_void_p(centers.data_ptr()), 2, None, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(grad.data_ptr()), None, None) == 1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((grad == SENTINEL).all())
    ctx.close()
    # outside the scope: nothing launched
    case, mocks, theta, _, _ = reference('cfg4_bao_xi')
    ctx = _context(case)
    ctx.set_data_batch(mocks[:NM])
    centers, index = _rows(theta)
    B, P = centers.shape
    hessian, gradient, offset, logposterior, grad = (torch.full(shape, SENTINEL, dtype=torch.float64, device=device) for shape in [(B, P, P), (B, P), (B,), (B,), (B, P)])
    status = torch.full((B,), -7, dtype=torch.int32, device=device)
    assert ctx.eval_fisher_analytic_data(_t(centers), _t(index), hessian=hessian, gradient=gradient, offset=offset) is None
    assert ctx.eval_logposterior_grad_data(_t(centers), _t(index), logposterior=logposterior, grad=grad, status=status) is None
    torch.cuda.synchronize()
    assert all(bool((tensor == SENTINEL).all()) for tensor in [hessian, gradient, offset, logposterior, grad]) and bool((status == -7).all())
    ctx.close()


# ---- 4. Python --------------------------------------------------------------------------------------------------------------------------
def test_fisher_evaluate_with_data_index():
    """``Fisher(method='analytic').evaluate(centers, data_index)`` on the marg_sn0_grid likelihood (sn0 varied) against ``Fisher(method='analytic').evaluate(centers)`` of
    per-mock likelihoods; 'finite' and 'auto' keep the finite route: the same bits from both."""
    import warnings
    from desilike_amd.fisher import Fisher
    g, like = _marg_likelihood()
    like.initialize()
    M = 3
    mocks = _marg_mocks(like, M)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fisher = Fisher(like, method='analytic')
        names = fisher.varied_params.names()
        assert 'sn0' in names
        rnames = [str(n) for n in g['names']]
        centers = np.ascontiguousarray(np.asarray(g['theta'], dtype='f8')[:NC][:, [rnames.index(name) for name in names if name in rnames]])
        if centers.shape[1] < len(names):      # (sn0 is solved in the fixture: its column is not in theta)
            centers = np.column_stack([centers] + [np.full(NC, fisher.varied_params[name].value) for name in names if name not in rnames])
        own = fisher.evaluate(centers)              # the analytic method accepts the likelihood
        assert all(np.isfinite(a).all() for a in own)
        assert fisher.set_data_batch(mocks) == M
        rows, index = np.repeat(centers, M, axis=0), np.tile(np.arange(M), NC)
        offset, gradient, hessian = fisher.evaluate(rows, data_index=index)
        assert np.array_equal(hessian, fisher.evaluate(rows)[2])      # the Hessian does not depend on the data: that of the same batch without a data index
        for m in range(M):
            ro, rg, rh = Fisher(_marg_likelihood(data=mocks[m])[1], method='analytic').evaluate(centers)
            for c in range(NC):
                row = c * M + m
                assert abs(offset[row] - ro[c]) <= 1e-9 + 1e-10 * abs(ro[c])
                assert np.abs(gradient[row] - rg[c]).max() <= 1e-8 * np.abs(rg[c]).max()
                assert np.abs(hessian[row] - rh[c]).max() <= 1e-11 * np.abs(rh[c]).max()      # (the bound of test_gpu_fisher_analytic.py::test_plumbing between batch sizes)
        finite, auto = Fisher(like, method='finite'), Fisher(like, method='auto')
        finite.set_data_batch(mocks); auto.set_data_batch(mocks)
        assert all(np.array_equal(a, b) for a, b in zip(finite.evaluate(rows, data_index=index), auto.evaluate(rows, data_index=index)))
        exact, differenced = (offset, gradient, hessian), finite.evaluate(rows, data_index=index)
        assert np.allclose(exact[0], differenced[0], rtol=1e-10, atol=1e-9)
        for a, f in zip(exact[1:], differenced[1:]):
            assert np.allclose(a, f, rtol=1e-3, atol=1e-5 * np.abs(a).max())      # (tests/test_gpu_fisher_analytic.py::test_fisher_analytic_vs_finite_cfg2)


def _central_differences(batch, values, index, scale):
    """(gradient [B, P], interval lower + upper [B, P]) by central differences of ``batch.logposterior`` with ``scale`` times the steps of the 'finite' method
    (``Parameter.delta``, shortened at the prior bounds)."""
    B, P = values.shape
    lower, upper = np.empty((B, P)), np.empty((B, P))
    for ip, param in enumerate(batch.likelihood.varied_params):
        _, lo, hi = param.delta
        lower[:, ip] = scale * np.clip(np.minimum(lo, values[:, ip] - param.prior.limits[0]), 0., None)
        upper[:, ip] = scale * np.clip(np.minimum(hi, param.prior.limits[1] - values[:, ip]), 0., None)
    points = np.repeat(values[:, None, :], 2 * P, axis=1)
    column = np.arange(P)
    points[:, 2 * column, column] -= lower
    points[:, 1 + 2 * column, column] += upper
    logpost = batch.logposterior(points.reshape(-1, P), np.repeat(index, 2 * P)).reshape(B, 2 * P)
    return (logpost[:, 1::2] - logpost[:, 0::2]) / (lower + upper), lower + upper


def test_data_batch_logposterior_grad():
    """``DataBatch.logposterior_grad``: 'analytic' against 'finite' (the bound of tests/test_fisher.py:195) and against ``logposterior``; 'auto' is 'analytic' here; on the
    marginalised sn0 likelihood the constant offset of the construction is carried."""
    from bench_configs import make_cfg2, make_cfg4
    for make, label in [(lambda: make_cfg2(), 'cfg2'), (lambda: _marg_likelihood(), 'marg_sn0')]:
        g, like = make()
        like.initialize()
        M, B = 4, 6      # (six rows of the marg_sn0_grid fixture lie inside the priors)
        flatdata = np.concatenate(like._flatdata_list())
        mocks = flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(5).standard_normal((M, flatdata.size))
        names, rnames = like.varied_params.names(), [str(n) for n in g['names']]
        values = np.ascontiguousarray(np.asarray(g['theta'], dtype='f8')[:, [rnames.index(name) for name in names]])
        batch = like.data_batch(mocks)
        paired_all = batch.logposterior(values, np.arange(len(values)) % M)
        inside = np.flatnonzero(np.isfinite(paired_all))[:B]
        assert len(inside) == B
        values, index = values[inside], (inside % M)
        value, grad = batch.logposterior_grad(values, index, method='analytic')
        value_fd, grad_fd = batch.logposterior_grad(values, index, method='finite')
        value_auto, grad_auto = batch.logposterior_grad(values, index)
        assert np.array_equal(value_auto, value) and np.array_equal(grad_auto, grad)
        assert (np.abs(value - paired_all[inside]) <= _tol(value)).all() and np.allclose(value, value_fd, rtol=1e-12, atol=1e-9)
        # 'finite' is off by its own truncation error, h^2 / 6 |f'''| to leading order, which the same stencil at half the steps measures: g(h) - g(h / 2) = 3 / 4 of
        # it.  Bound: twice that estimate (the next order), plus the rounding of a difference of two log-posteriors good to 1e-10 max(1, |logL|) over the half step.
        full, half = _central_differences(batch, values, index, 1.), _central_differences(batch, values, index, 0.5)
        assert (np.abs(full[0] - grad_fd) <= 4e-10 * np.maximum(1., np.abs(value))[:, None] / full[1]).all()      # (the stencil of the 'finite' method itself, in another batch)
        truncation = 4. / 3. * np.abs(full[0] - half[0])
        bound = 2. * truncation + 2e-10 * np.maximum(1., np.abs(value))[:, None] / (0.5 * full[1])
        print('{}: DataBatch.logposterior_grad analytic against finite: up to {:.2e} of the largest component, {:.2e} of the bound from the truncation of the differences'.format(
            label, np.abs(grad - grad_fd).max() / np.abs(grad).max(), (np.abs(grad - grad_fd) / bound).max()))
        assert (np.abs(grad - grad_fd) <= bound).all(), (np.abs(grad - grad_fd) / bound).max()
        if label == 'cfg2': assert np.allclose(grad, grad_fd, rtol=1e-3, atol=1e-5 * np.abs(grad).max())      # (the bound of tests/test_fisher.py:195 on its configuration)
        if label == 'marg_sn0': assert batch.offset != 0.
    # outside the scope: 'analytic' raises, 'auto' is 'finite'
    g4, like4 = make_cfg4('pk')
    like4.initialize()
    flatdata = np.concatenate(like4._flatdata_list())
    batch = like4.data_batch(np.vstack([flatdata, 1.01 * flatdata]))
    values = np.ascontiguousarray(np.asarray(g4['theta'], dtype='f8')[:4, [[str(n) for n in g4['names']].index(name) for name in like4.varied_params.names()]])
    index = np.arange(4) % 2
    with pytest.raises(NotImplementedError, match='finite'):
        batch.logposterior_grad(values, index, method='analytic')
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(batch.logposterior_grad(values, index), batch.logposterior_grad(values, index, method='finite')))
