"""GPU (-m gpu): the marginalised finalize at EVERY number of solved parameters n_s = 1 .. 16, on every solve route of ``dl_launch_finalize_marg`` (csrc/dl_kernels.hip) and of the
fused tails (csrc/dl_emu_batch.h), against the extended-precision reference of tests/marg_reference.py on 8 rows per case.  The cases and their oracle-side inputs (Delta(x0) and T
from the oracle's theory chain, data = the oracle's theory at a drawn point + one noise draw) live in tests/marg_counts_cases.py; tests/test_marg_reference.py shows on the CPU that
every case has chi2(x0) <= 1e4 and is solved by the float64 oracle to 1e-11, so that the project's tolerances below test the kernels.

Residual route (EFT-like Kaiser, one to three tracers, dense window and cross-covariance; counter terms = point-dependent rows, stochastic terms = constant rows):
  n = 57 (no multiple of 4) with n_s = 1 .. 16; n = 20 (the 512-double floor of a wave's staging region) with n_s = 1, 3; n = 120 with n_s = 11, 12 (47 616 / 51 584 B of LDS: either
  side of the 48 KB above which the launch needs hipFuncSetAttribute); n = 360 with n_s = 7, 8 (93 184 / 104 832 B: either side of 96 KB, staged / unstaged); n = 504 and 512 (the
  limit) with n_s = 4, 5, 15, 16.  The branch is computed here with the dispatch's own formula and printed: staged<true,true>, the same above 48 KB, unstaged<true,false> chosen by
  size, serial<false,false> (n_s = 16).
Gram route (one emulated observable; G comes out of the feature GEMM): ``make_mlp_likelihood`` with n_s = 1 .. 6 in the 'physical' basis and 7 in the 'standard' basis, the Taylor
  variant ``make_cfg3`` with 1 .. 6; each through the fused tail, DL_NO_FUSED_SOLVE=1 (dl_finalize_marg_gram_kernel<NS>) and DL_FM_NO_LANE_SOLVE=1 (dl_finalize_marg_kernel<true,false>
  reading G).
UNREACHABLE from any context the library can create: ``dl_finalize_marg_gram_kernel<8>`` and the ready-Gram branch of ``dl_finalize_marg_kernel<true,false>`` at n_s = 9 .. 15 (that
  branch runs at n_s <= 7 under DL_FM_NO_LANE_SOLVE=1 only).  A Gram matrix is only ever formed for ONE emulated observable on the feature path; the linear inputs of an emulated
  theory are the seven velocileptors terms alpha0 alpha2 alpha4 alpha6 sn0 sn2 sn4 (DL_STK_ROWS = 8 likewise), and pass-through columns of the window -- the only other
  source of linear parameters -- switch the feature path off in dl_create (n_pass != 0).  Editing the key set cannot add what the theory kernel has no input for.

Every case: the '.marg' patterns all / none / first / last / alternating / a seeded random half; Gaussian priors with loc != x0 mixed with flat ones; batches of 1, 3, 5, 64, 65 rows
and one on each side of the point where ``dl_gemm_tiled_splits`` first returns 1 -- with its tiles of DL_GT_M x DL_GT_N = 64 x 128 and the target of 256 workgroups
(csrc/dl_gemm_tiled.h, dl_kernels.hip), S = min(max(256 / tiles, 1), min(K_pad / 16, 32)) is 1 from tiles = ceil(M / 64) (N_pad / 128) = 129 on, i.e. from M = B (1 + n_var) = 8193 rows of
the window GEMM at N_pad = 128 (2049 at N_pad = 512): the 4-point workgroups of the finalize see spare waves, the 64-point ones a ragged tail, and the finalize sums 32 .. 2 slabs or reads one.
The same row in two batches with the same split count must agree bit for bit, with different split counts to 1e-12 max(1, |.|)."""
import os

import numpy as np
import pytest

import marg_reference as mr
import marg_counts_cases as mc

pytestmark = pytest.mark.gpu

DL_ST_NONFINITE = 2


def tiled_splits(M, N_pad, K_pad):
    """``dl_gemm_tiled_splits`` (csrc/dl_kernels.hip): split-K slabs of the window GEMM of M rows."""
    GT_M, GT_N, GT_K, GT_PANEL, target = 64, 128, 16, 6, 256
    tiles, nchunks = -(-M // GT_M) * (N_pad // GT_N), K_pad // GT_K
    if tiles <= target: return min(max(target // tiles, 1), min(nchunks, 32))
    cost = lambda s: -(-tiles * s // target) * (-(-nchunks // s) + 12.)   # noqa: E731
    return 2 if nchunks >= 2 * GT_PANEL and cost(2) < 0.95 * cost(1) else 1


def split_point(R, N_pad, K_pad):
    """Smallest batch whose window GEMM (R rows per point) is not split."""
    B = 1
    while tiled_splits(B * R, N_pad, K_pad) != 1: B += 1
    return B


def reference_rows(case, patterns):
    """{pattern: [reference of each compared row]}: one exact Gram matrix per row, shared by the patterns."""
    precision = mr.exact_ints(case.precision)
    grams = [mr.marg_gram(case.delta[i], case.T[i], precision) for i in range(mc.NROWS)]
    return {name: [mr.marg_from_gram(G, case.x0, case.prior_loc, case.prior_scale, mask) for G in grams] for name, mask in patterns}


def compare(out, refs, logprior_varied, label):
    """Outputs of ``eval_batch_derived_host`` on the first rows of a batch against the reference, at the project's tolerances; returns the largest relative errors."""
    loglike, logprior, status, solved, hessian = out
    nrows = min(len(loglike), mc.NROWS)
    assert (status[:nrows] == 0).all(), (label, status[:nrows])
    errs = np.zeros(4)
    for i in range(nrows):
        ref = refs[i]
        lp_ref = logprior_varied[i] + ref['logprior_solved']
        hmax = np.abs(ref['likelihood_hessian']).max()
        e = [abs(loglike[i] - ref['loglikelihood']) / max(1., abs(ref['loglikelihood'])), abs(logprior[i] - lp_ref) / max(1., abs(lp_ref)),
             (np.abs(solved[i] - ref['x']) / (1e-10 + 1e-8 * np.abs(ref['x']))).max(), (np.abs(hessian[i] - ref['likelihood_hessian']) / (1e-12 * hmax + 1e-10 * np.abs(ref['likelihood_hessian']))).max()]
        errs = np.maximum(errs, e)
        assert e[0] <= 1e-10, (label, i, 'loglike', loglike[i], ref['loglikelihood'], e[0])
        assert e[1] <= 1e-10, (label, i, 'logprior', logprior[i], lp_ref, e[1])
        assert np.allclose(solved[i], ref['x'], rtol=1e-8, atol=1e-10), (label, i, 'solved', solved[i], ref['x'])
        assert np.allclose(hessian[i], ref['likelihood_hessian'], rtol=1e-10, atol=1e-12 * hmax), (label, i, 'hessian', e[3])
    return errs     # (loglike and logprior: relative; solved and Hessian: in units of their tolerance)


def compare_batches(outs, splits, label):
    """The compared rows across batches: bit for bit at equal split count, 1e-12 max(1, |.|) otherwise."""
    sizes = sorted(outs)
    for a in sizes:
        for b in sizes:
            if b <= a: continue
            nrows = min(a, b, mc.NROWS)
            for qa, qb in zip(outs[a], outs[b]):
                qa, qb = qa[:nrows], qb[:nrows]
                if splits[a] == splits[b]: assert np.array_equal(qa, qb), (label, a, b, splits[a], np.abs(qa - qb).max())
                else: assert (np.abs(qa - qb) <= 1e-12 * np.maximum(1., np.abs(qb))).all(), (label, a, b, splits[a], splits[b], np.abs(qa - qb).max())


def batch(case, size, filler):
    return np.ascontiguousarray(np.concatenate([case.theta, filler])[:size] if size > mc.NROWS else case.theta[:size])


@pytest.mark.parametrize('n,n_s', mc.CASES, ids=mc.CASE_IDS)
def test_residual_route(n, n_s):
    from desilike_amd._lib import Context
    case = mc.get_case(n, n_s)
    patterns = mc.mask_patterns(n_s, seed=n_s)
    refs = reference_rows(case, patterns)
    like = case.likelihood(np.ones(n_s, dtype='?'))
    like.initialize()
    assert like.solved_params.names() == case.solved and like.varied_params.names() == case.names
    spec = like._spec({}, like._flatdata_list(), like._precision_input)
    assert np.array_equal(spec['marg']['kind'], np.ones(n_s)) and np.array_equal(spec['marg']['x0'], case.x0)
    logprior_varied = case.logprior_varied(case.theta)
    rng = np.random.RandomState(n + n_s)
    R = 1 + case.n_var
    branch, shm = mc.expected_branch(n, n_s), mc.staged_lds_bytes(n, n_s)
    worst = np.zeros(4)
    for ip, (name, mask) in enumerate(patterns):
        # the first pattern through the likelihood's own context (flags '.marg'); the others change marg.kind alone ('.best' through the Python layer: tests/test_gpu_marg.py)
        ctx = like._get_context() if ip == 0 else Context(dict(spec, marg=dict(spec['marg'], kind=mask.astype('i4'))), device=like.device)
        assert ctx.n_solved == n_s and ctx.n_data == n
        N_pad, K_pad = ctx.info('N_pad'), ctx.info('K_pad')
        B1 = split_point(R, N_pad, K_pad)
        sizes = [1, 3, 5, 64, 65, B1 - 1, B1]
        filler = np.column_stack([np.clip(param.ref.sample(size=max(sizes), random_state=rng), *param.prior.limits) for param in like.varied_params])
        outs, splits = {}, {}
        for size in sizes:
            out = ctx.eval_batch_derived_host(batch(case, size, filler))
            splits[size] = tiled_splits(size * R, N_pad, K_pad)
            worst = np.maximum(worst, compare(out, refs[name], logprior_varied, (n, n_s, name, size)))
            outs[size] = (out[0], out[1], out[3], out[4])
        assert splits[B1 - 1] > 1 and splits[B1] == 1, splits
        compare_batches(outs, splits, (n, n_s, name))
        if ip > 0: ctx.close()
    print('\nresidual n = {:3d} n_s = {:2d} n_var = {:d} {:28s} LDS {:6d} B  N_pad {:d} K_pad {:d} unsplit from B = {:d}  {:d} patterns  max err: loglike {:.1e} logprior {:.1e} solved {:.2f} tol hessian {:.2f} tol'
          .format(n, n_s, case.n_var, branch, shm if n_s < 16 else 0, N_pad, K_pad, B1, len(patterns), *worst))


def _set(**env):
    from desilike_amd._lib import refresh_options
    for key, value in env.items():
        if value is None: os.environ.pop(key, None)
        else: os.environ[key] = value
    refresh_options()


GRAM_VARIANTS = [('fused tail', {}), ('gram_kernel<NS>', {'DL_NO_FUSED_SOLVE': '1'}), ('16 lanes per point on G', {'DL_NO_FUSED_SOLVE': '1', 'DL_FM_NO_LANE_SOLVE': '1'})]


@pytest.mark.parametrize('kind,basis,count', mc.GRAM_CASES, ids=mc.GRAM_CASE_IDS)
def test_gram_route(kind, basis, count):
    from desilike_amd._lib import Context
    case = mc.get_gram_case(kind, basis, count)
    patterns = mc.mask_patterns(count, seed=count)
    refs = reference_rows(case, patterns)
    logprior_varied = case.logprior_varied(case.theta)
    rng = np.random.RandomState(count)
    sizes = [1, 3, 5, 64, 65, 200]
    worst = {label: np.zeros(4) for label, env in GRAM_VARIANTS}
    for name, mask in patterns:
        like = case.likelihood(mask)       # the flags through the Python layer
        like.initialize()
        assert like.solved_params.names() == case.solved and like.varied_params.names() == case.names
        ctx = Context(like._spec({}, [case.flatdata], like._precision_input), device=like.device)
        assert ctx.n_solved == count and ctx.info('N_pad') == 128
        filler = np.column_stack([np.clip(param.ref.sample(size=max(sizes), random_state=rng), *param.prior.limits) for param in like.varied_params])
        for label, env in GRAM_VARIANTS:
            _set(**env)
            try:
                outs = {size: ctx.eval_batch_derived_host(batch(case, size, filler)) for size in sizes}
            finally:
                _set(**{key: None for key in env})
            for size, out in outs.items():
                worst[label] = np.maximum(worst[label], compare(out, refs[name], logprior_varied, (kind, basis, count, name, label, size)))
            compare_batches({size: (out[0], out[1], out[3], out[4]) for size, out in outs.items()}, {size: 1 for size in sizes}, (kind, basis, count, name, label))
        ctx.close()
    print()
    for label, errs in worst.items():
        print('gram {:6s} {:8s} n_s = {:d} {:24s} {:d} patterns  max err: loglike {:.1e} logprior {:.1e} solved {:.2f} tol hessian {:.2f} tol'.format(kind, basis, count, label, len(patterns), *errs))


def _singular_residual():
    """One solved parameter with a flat prior and an exactly zero derivative row: sn4_2 (k^2 in the hexadecapole) with a window whose hexadecapole input columns are zero."""
    import bench
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, EFTLikeKaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    theory = EFTLikeKaiserTracerPowerSpectrumMultipoles(template=ShapeFitPowerSpectrumTemplate(z=0.8, fiducial='synthetic'))
    for name in ['ct0_2', 'ct2_2', 'ct4_2', 'sn0_2', 'sn2_2']: theory.init.params[name].update(fixed=True, value=0.)
    theory.init.params['sn4_2'].update(derived='.marg', prior=dict(dist='uniform'))
    kedges = np.linspace(0.02, 0.2, 11)
    kin, full = bench.dense_window(kedges, (0, 2, 4), resolution=2, seed=3)
    wmatrix = full[:20].copy()                       # data: ell = (0, 2)
    wmatrix[:, 2 * len(kin):] = 0.                   # nothing of the theory's hexadecapole reaches the data
    obs = TracerPowerSpectrumMultipolesObservable(data=5e3 + 100. * np.random.RandomState(1).standard_normal(20), kedges=kedges, ells=(0, 2), wmatrix=wmatrix, kin=kin, ellsin=(0, 2, 4), theory=theory, shotnoise=1e4)
    return ObservablesGaussianLikelihood(observables=[obs], covariance=bench.synthetic_covariance(20, seed=4))


@pytest.mark.parametrize('route', ['residual', 'gram'])
def test_singular_system(route):
    """A flat-prior solved parameter whose derivative row is exactly zero: -H = 0 is not positive definite.  Every row reports DL_ST_NONFINITE, the log-posterior is -inf, nothing faults.
    Gram route: sn4p reaches only the hexadecapole rows of the data; the rows of the window matrix that produce them are zeroed in the key set (the Python layer has no such window)."""
    from desilike_amd._lib import Context
    if route == 'residual':
        like = _singular_residual()
        like.initialize()
        assert like.solved_params.names() == ['sn4_2']
        ctx = like._get_context()
    else:
        from test_gpu_emulator import make_mlp_likelihood
        g, like, pt, theory, solved = make_mlp_likelihood(marg=True, derived={'sn4p': '.marg'})
        theory.init.params['sn4p'].update(fixed=False, prior=dict(dist='uniform'))
        like.initialize()
        assert like.solved_params.names() == ['sn4p']
        spec = like._spec({}, like._flatdata_list(), like._precision_input)
        obs = dict(spec['observables'][0])
        wmatrix = np.array(obs['wmatrix'])
        assert wmatrix.shape[0] == 108
        wmatrix[72:] = 0.
        obs['wmatrix'] = wmatrix
        ctx = Context(dict(spec, observables=[obs]), device=like.device)
    assert ctx.n_solved == 1
    rng = np.random.RandomState(2)
    theta = np.column_stack([np.clip(param.ref.sample(size=67, random_state=rng), *param.prior.limits) for param in like.varied_params])
    variants = [{}] if route == 'residual' else [env for label, env in GRAM_VARIANTS]
    for env in variants:
        _set(**env)
        try:
            status = ctx.eval_batch_host(theta)[2]
            logpost, status_p = ctx.eval_logposterior_host(theta)
        finally:
            _set(**{key: None for key in env})
        assert (status == DL_ST_NONFINITE).all() and (status_p == DL_ST_NONFINITE).all(), (route, env, status)
        assert np.isneginf(logpost).all()


def test_dl_create_refusals():
    """dl_create refuses 17 solved parameters, and 513 data points with a solved parameter (the finalize keeps n / 64 <= 8 residual entries per lane)."""
    like = mc.build(57, 17)[0]
    like.initialize()
    assert len(like.solved_params) == 17
    with pytest.raises(Exception, match='at most 16 analytically solved parameters'):
        like._get_context()
    like = mc.build(513, 1)[0]
    like.initialize()
    assert len(like.solved_params) == 1 and len(like.flatdata) == 513
    with pytest.raises(Exception, match='analytic marginalisation supports up to 512 data points'):
        like._get_context()
    like = mc.build(512, 1)[0]      # the limit itself is served (tests above: n = 512)
    assert like._get_context().n_data == 512
