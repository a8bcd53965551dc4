"""GPU (-m gpu): the moment form of the fast full-shape theory kernels (csrc/dl_fullshape.h: dl_spline_eval_m, dl_fs_mom_fixup, dl_fs_knots_rec) -- the spline evaluated
from (knot value, moment) records, rows stored by the evaluating threads -- against the NumPy oracle and against the interval-polynomial path of the same library
(``DL_FS_NO_MOMENTS=1``), on batches of 5 and 37 points.  Batches this small take the 512-thread form of the kernel; a child process under ``DL_FS_WIDE=0`` (read once
per process) runs the same assertions on the 256-thread form: two wavenumbers per thread with a partly filled second half at 400 wavenumbers, three rounds of prefetched
knot records, the 192-thread tiling of the convolution.

Shapes: multipoles (0, 2, 4) on 400 wavenumbers and (0, 2) on 70 (threads without a wavenumber; dn varied there: the knot stage without the folded records).  Tables:
the default ``logspace(-3, 1, 400)`` (wavenumbers from 5e-4: evaluations below the first knot -- the first interval extrapolated -- and inside the first DL_FIR_PAD = 32
knots, where the end corrections live; the rest in the interior) and a 300-knot table ending at k = 0.3 (wavenumbers up to 0.35: inside the last 32 knots, from k = 0.163,
and beyond the last knot).  Points: qpar, qper and dm at the ends of their prior ranges in the first four rows, the others spread over the prior ranges.

Tolerances: 1e-10 on log-likelihoods against the oracle (relative above 1: the suite's); the two paths agree to 1e-12 of the row's largest magnitude on the theory vector."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path[:0] = [d for d in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),) if d not in sys.path]   # (the child process is started as a script)

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = {'l024-k400': dict(ells=(0, 2, 4), nk=400, vary_dn=False), 'l02-k70': dict(ells=(0, 2), nk=70, vary_dn=True)}
TABLES = {'default': None, 'ends-at-0.3': np.logspace(-3., np.log10(0.3), 300)}


def build(ells, nk, vary_dn, k_t=None, seed=4):
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    rng = np.random.RandomState(seed)
    kout = np.arange(0.025, 0.33, 0.02)
    kin = np.linspace(5e-4, 0.35, nk)
    nout = len(ells) * len(kout)
    wmat = np.abs(rng.standard_normal((nout, len(ells) * nk))) * 0.02      # every input wavenumber reaches the data: both ends of the table count
    for ill in range(len(ells)):
        for i, kk in enumerate(kout):
            wmat[ill * len(kout) + i, ill * nk + np.argmin(np.abs(kin - kk))] += 1.
    wmat /= wmat.sum(axis=1)[:, None]
    tpl = ShapeFitPowerSpectrumTemplate(z=0.8) if k_t is None else ShapeFitPowerSpectrumTemplate(z=0.8, k=k_t)
    if vary_dn: tpl.init.params['dn'].update(fixed=False)
    theory = KaiserTracerPowerSpectrumMultipoles(template=tpl)
    obs = TracerPowerSpectrumMultipolesObservable(data={'b1': 1.7}, k=kout, ells=ells, wmatrix=wmat, kin=kin, ellsin=ells, theory=theory, shotnoise=2e3)
    A = rng.standard_normal((nout, nout)) * 15.
    like = ObservablesGaussianLikelihood(observables=[obs], covariance=A.dot(A.T) + 1e4 * np.eye(nout))
    like.initialize()
    assert theory.k.size == nk
    return like, obs, theory, tpl


def points(like, n, seed=11):
    """n rows over the prior ranges; rows 0-3: qpar, qper, dm at the ends of their ranges"""
    rng = np.random.RandomState(seed)
    params = list(like.varied_params)
    names = [param.name for param in params]
    lo, hi = np.array([param.prior.limits[0] for param in params]), np.array([param.prior.limits[1] for param in params])
    ref = np.array([param.value for param in params])
    # AP and shape parameters over their whole prior ranges, the others (df, b1, sn0: wide or unbounded priors) around their values
    wide = np.array([name in ('qpar', 'qper', 'dm', 'dn') for name in names])
    theta = np.where(wide, rng.uniform(np.where(wide, lo, 0.), np.where(wide, hi, 1.), size=(n, len(params))), ref * rng.uniform(0.9, 1.1, size=(n, len(params))) + rng.uniform(-0.05, 0.05, size=(n, len(params))))
    ends = [(0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 0)]
    for row, (a, b, c) in enumerate(ends):
        for name, e in zip(['qpar', 'qper', 'dm'], (a, b, c)):
            i = names.index(name)
            theta[row, i] = (lo[i], hi[i])[e]
    return names, theta


def oracle_constants(obs, theory, tpl):
    wm = obs.wmatrix
    return dict(template='shapefit', k11=tpl.k, pk_dd_fid=tpl.pk_dd_fid, f_fid=tpl.f_fid, kp=tpl.kp, a=tpl.a, kin=theory.k, mu=theory.mu, wmu_ell=theory.wmu,
                ellsin=theory.ells, nd=theory.nd, matrix_full=wm.matrix_full, kmask=wm.kmask, offset=wm.offset, shotnoisein=wm.shotnoisein, shotnoiseout=wm.shotnoiseout,
                flatdata=obs.flatdata)


class Case:
    """One (shape, table): the likelihood, its 37 points and their oracle log-likelihoods, computed once"""
    cache = {}

    @classmethod
    def get(cls, shape, table, k_t=None):
        key = (shape, table)
        if key not in cls.cache:
            like, obs, theory, tpl = build(k_t=TABLES[table] if k_t is None else k_t, **SHAPES[shape])
            names, theta = points(like, 37)
            c = oracle_constants(obs, theory, tpl)
            ref = []
            for row in theta:
                p = dict(zip(names, row)); p['b1'] = (p['b1'], p['b1'])
                ref.append(orc.gaussian_loglikelihood(orc.fullshape_observable(c, p)['flattheory'], obs.flatdata, like.precision)[0])
            cls.cache[key] = (like, theta, np.array(ref))
        return cls.cache[key]


def check_loglike(ctx, theta, ref):
    for B in (5, 37):
        loglike, logprior, status = ctx.eval_batch_host(theta[:B])
        err = np.abs(loglike - ref[:B]) / np.maximum(1., np.abs(ref[:B]))
        print('batch {:d}: largest log-likelihood error {:.3g}'.format(B, err.max()))
        assert (status == 0).all() and (err <= 1e-10).all(), (B, float(err.max()))


def run_case(shape, table):
    from desilike_amd._lib import refresh_options
    like, theta, ref = Case.get(shape, table)
    ctx = like._get_context()
    assert ctx.info('moment_form_obs0') == (1 if SHAPES[shape]['vary_dn'] else 3)      # the moment form is what runs (with the folded knot records where dn is constant)
    check_loglike(ctx, theta, ref)
    moments = [ctx.eval_theory_host(theta[:B], iobs=0) for B in (5, 37)]
    os.environ['DL_FS_NO_MOMENTS'] = '1'; refresh_options()
    try:
        polynomial = [ctx.eval_theory_host(theta[:B], iobs=0) for B in (5, 37)]
    finally:
        del os.environ['DL_FS_NO_MOMENTS']; refresh_options()
    for got, parent in zip(moments, polynomial):
        rows = parent.reshape(parent.shape[0], -1)
        err = np.abs(got.reshape(rows.shape) - rows).max(axis=1) / np.abs(rows).max(axis=1)
        print('{:d} rows: largest difference between the paths {:.3g} of the row maximum'.format(rows.shape[0], err.max()))
        assert (err <= 1e-12).all(), float(err.max())
    assert not np.array_equal(moments[1], polynomial[1])      # (the switch did select another path)


@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_moment_form_vs_oracle_and_vs_polynomial_path(shape, table):
    run_case(shape, table)


def test_the_256_thread_form_in_a_child_process():
    """DL_FS_WIDE is read once per process: the child runs every (shape, table) on dl_fullshape_kernel instead of the 512-thread form of small batches."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, DL_FS_WIDE='0'), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(out.stdout.decode()[-2000:])
    assert out.returncode == 0 and 'every case ok' in out.stdout.decode(), out.stderr.decode()[-2000:]


def test_perturbed_knot_tables_keep_the_polynomial_path():
    """The moment form evaluates on the exactly uniform grid, so it must refuse knots that are off it.  By 1e-9 in log10 k (1e-7 of the spacing): not even a convolution
    table, the general kernel runs.  By 3e-14 (3e-12 of the spacing, below the 1e-11 the convolution accepts): the fast kernel, where only the bound on
    g max|dlt| inv_hx (about 5e-13 here against 1e-14) keeps the interval polynomials, which carry the shift.  Both still meet the oracle."""
    rng = np.random.RandomState(2)
    for name, eps in [('perturbed-1e-9', 1e-9), ('perturbed-3e-14', 3e-14)]:
        k_t = 10.**(np.linspace(-3., 1., 400) + eps * rng.uniform(-1., 1., size=400))
        like, theta, ref = Case.get('l024-k400', name, k_t=k_t)
        ctx = like._get_context()
        assert ctx.info('moment_form_obs0') == 0, name
        check_loglike(ctx, theta, ref)


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    assert os.environ.get('DL_FS_WIDE') == '0'
    for shape in SHAPES:
        for table in TABLES:
            print(shape, table)
            run_case(shape, table)
    print('every case ok')
