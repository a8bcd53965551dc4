"""GPU (-m gpu): the prior record of the plain-likelihood chi2-GEMM step (csrc/dl_prior.h: ``dl_prior_record``, written by the theory kernel that opens the step;
``dl_finalize_rec_kernel`` then only sums the partial chi2) against the finalize that evaluates the priors itself (``dl_finalize_part_kernel``, reached through
``DL_FS_NO_PRIOR=1`` + ``dl_options_refresh``) -- ``loglike``, ``logprior``, ``status`` and the log-posterior BIT FOR BIT -- and against ``oracle.np_oracle.logprior``
at 1e-12 max(1, |logprior|).

Contexts (built once, shared by the tests).  Parameter counts: 1 (only ``b1`` of the ShapeFit + Kaiser fixture varied), 6 (that fixture as it is: the shape of the
benchmark's headline), 8 and 9 (the second group of eight of the old kernel's ``dl_load_theta8``), 15 (the EFT fixture: counter terms, the EFT instantiation) and 26
(the "more than 25 parameters" loop of the old kernel's LDS stage).  The theory kernels read at most 8 counter-term and 8 stochastic parameters (``DL_MAX_EFT``)
next to 8 template / bias parameters; the fixtures carry 6 and 15 parameters THROUGH the theory, which is the largest count tested that way -- the columns that bring
the count to 8, 9 and 26 are varied parameters with priors that no observable reads (the priors are what is under test).  Prior kinds: uniform and normal, with and
without finite limits.  Two observables: ``boundary_two_tracers`` at 32 and 33 points, merged launch and one launch per observable (``DL_NO_MERGED_THEORY``).

Batch sizes 1, 31, 33, 65, 256 (the 512-thread theory form; the ends of the 32-row GEMM block and of the 64-thread finalize workgroup) and 257 (the 256-thread
form).  Rows 1-7, 32, 64 and 256 of every batch that holds them are special: a parameter exactly on a closed limit (status 0), NaN in the first / middle / last
parameter (3), a parameter outside its limits (1, logprior -inf, posterior -inf), a non-finite chi2 with finite priors (2), NaN together with a parameter outside (3).
Outputs are written into oversized device buffers: nothing beyond row B - 1 may change.  Null output pointers, posterior mode, the forced GEMM tile heights
``DL_CG_MT=16 / 32`` and the fused forms ``DL_CHI2_FUSED=1`` / ``DL_STEP_KERNEL=1`` (256 points; against the
default under ``DL_FS_NO_MOMENTS=1``, the theory path that kernel runs) are compared with the default bit for bit.  Child processes (switches
read once per process) repeat the comparison on the 256-thread and DENSE forms at small batches (``DL_FS_WIDE=0 DL_FS_DENSE_MIN=256``) and on the generic kernel
(``DL_NO_TOEPLITZ=1``)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [d for d in (os.path.dirname(HERE), HERE) if d not in sys.path]   # (the child process is started as a script)

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 33, 65, 256, 257)
BMAX = max(BATCHES)
EXTRA = np.array([[1., -5., 5., 0.3, 2.], [0., -1., 1., 0., 1.], [1., -np.inf, np.inf, -0.2, 0.7]])   # priors of the columns no observable reads, in turn
HUGE = 1e153       # a normal prior of scale >= 1 stays finite there ((1e153)^2 = 1e306), the chi2 of a theory vector that carries it does not


@contextlib.contextmanager
def switches(**env):
    from desilike_amd._lib import refresh_options
    os.environ.update(env); refresh_options()
    try:
        yield
    finally:
        for name in env: del os.environ[name]
        refresh_options()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u8') if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Case:
    """One context: its prior table, BMAX points with the special rows, what the special rows must give, the oracle's log-priors"""
    cache = {}

    def __init__(self, name):
        from desilike_amd._lib import Context
        from golden_utils import load_golden, spec_from_golden
        rng = np.random.RandomState(7)
        huge = None
        if name == 'two':
            from test_gpu_boundary import load_fixture
            g, cfg = load_fixture('two_tracers')
            spec = {key: np.array(value) for key, value in cfg.items()}
            priors, rows = np.reshape(cfg['priors'], (-1, 5)).astype('f8'), np.asarray(g['theta'], dtype='f8')
        else:
            g = load_golden('cfg2v_eft_damping_qisoqap' if name in ('p15', 'p26') else 'cfg2_shapefit_window')
            names = [str(n) for n in g['names']]
            spec = spec_from_golden(g)
            priors, rows = np.reshape(g['priors'], (-1, 5)).astype('f8'), np.asarray(g['theta'], dtype='f8')
            huge = names.index('sn0')
            if name == 'p1':      # b1 alone, a normal prior inside closed limits; every other input at the value of the fixture's first row
                i = names.index('b1')
                obs = dict(spec['observables'][0])
                obs['inputs'] = {key: ((0, const) if col == i else (-1, rows[0, col] if col >= 0 else const)) for key, (col, const) in obs['inputs'].items()}
                spec = dict(spec, observables=[obs])
                priors, rows, huge = np.array([[1., 0., 4., 1.7, 0.5]]), rows[:, [i]], None
            n_extra = int(name[1:]) - len(priors)
            assert n_extra >= 0
            priors = np.vstack([priors] + [EXTRA[[j % len(EXTRA)]] for j in range(n_extra)])
            spec = dict(spec, n_params=np.array([len(priors)]), priors=priors)
        self.name, self.priors, P = name, priors, len(priors)
        n_theory = rows.shape[1]
        inside = ((rows >= priors[:n_theory, 1]) & (rows <= priors[:n_theory, 2])).all(axis=1) & np.isfinite(rows).all(axis=1)
        rows = rows[inside]
        i, j, a = rng.randint(len(rows), size=BMAX), rng.randint(len(rows), size=BMAX), rng.uniform(size=(BMAX, 1))
        theta = np.empty((BMAX, P))
        theta[:, :n_theory] = a * rows[i] + (1. - a) * rows[j]          # (the priors are boxes)
        for col in range(n_theory, P):
            kind, lo, hi, loc, scale = priors[col]
            theta[:, col] = rng.uniform(lo, hi, size=BMAX) if np.isfinite(lo) else loc + scale * rng.standard_normal(BMAX)
        lo_col = int(np.flatnonzero(np.isfinite(priors[:, 1]))[0])
        hi_col = int(np.flatnonzero(np.isfinite(priors[:, 2]))[-1])
        self.expect = {}      # row -> status
        theta[1, lo_col] = priors[lo_col, 1]; self.expect[1] = 0
        for row, col in [(2, 0), (3, P // 2), (4, P - 1), (64, 0)]: theta[row, col] = np.nan; self.expect[row] = 3
        for row, d in [(5, 0.5), (32, 1e-12), (256, 7.)]: theta[row, hi_col] = priors[hi_col, 2] + d; self.expect[row] = 1
        if huge is not None: theta[6, huge] = HUGE; self.expect[6] = 2
        theta[7, lo_col] = priors[lo_col, 1] - 1.; theta[7, P - 1] = np.nan; self.expect[7] = 3
        self.theta = theta
        prior_list = [dict(dist=['uniform', 'norm'][int(row[0])], limits=(row[1], row[2]), loc=row[3], scale=row[4]) for row in priors]
        with np.errstate(invalid='ignore'):
            self.oracle_logprior = orc.logprior(theta, prior_list)
        self.ctx = Context(spec, device=0)
        assert self.ctx.n_params == P
        self.theta.setflags(write=False); self.oracle_logprior.setflags(write=False)

    @classmethod
    def get(cls, name):
        if name not in cls.cache: cls.cache[name] = cls(name)
        return cls.cache[name]


def evaluate(case, B):
    """(loglike, logprior, status, logposterior, status of the posterior call) of the first B points through the host-array entry points"""
    return case.ctx.eval_batch_host(case.theta[:B]) + case.ctx.eval_logposterior_host(case.theta[:B])


def check_batch(case, B, label=''):
    new = evaluate(case, B)
    with switches(DL_FS_NO_PRIOR='1'):
        old = evaluate(case, B)
    for got, ref, what in zip(new, old, ['loglike', 'logprior', 'status', 'logposterior', 'status (posterior call)']):
        assert same_bits(got, ref), (case.name, label, B, what, np.flatnonzero(bits(got) != bits(ref))[:8])
    loglike, logprior, status, post, status_post = new
    assert np.array_equal(status, status_post)
    ref = case.oracle_logprior[:B]
    finite = np.isfinite(ref)
    err = np.abs(logprior[finite] - ref[finite]) / np.maximum(1., np.abs(ref[finite]))
    print('{} {} B = {:d}: largest log-prior error against the oracle {:.3g}'.format(case.name, label, B, err.max() if err.size else 0.))
    assert (err <= 1e-12).all() and np.isneginf(logprior[~finite]).all() and np.isneginf(ref[~finite]).all(), (case.name, B)
    special = {row: st for row, st in case.expect.items() if row < B}
    ordinary = np.array([row not in special for row in range(B)])
    assert (status[ordinary] == 0).all() and np.isfinite(loglike[ordinary]).all()
    assert same_bits(post[ordinary], loglike[ordinary] + logprior[ordinary])
    for row, st in special.items():
        assert status[row] == st, (case.name, B, row, status[row], st)
        if st == 0: assert np.isfinite(logprior[row]) and post[row] == loglike[row] + logprior[row]
        else: assert np.isneginf(post[row])
        if st in (1, 3): assert np.isneginf(logprior[row])
        if st == 2: assert np.isfinite(logprior[row]) and not np.isfinite(loglike[row])


def check_device_outputs(case, B):
    """Device tensors: outputs in oversized buffers (nothing beyond row B - 1 is written), then every output pointer null but one"""
    import torch
    device = torch.device('cuda', 0)
    theta = torch.as_tensor(case.theta[:B].copy(), device=device)
    pad = 64

    def buffers():
        return torch.full((B + pad,), -7.25, dtype=torch.float64, device=device), torch.full((B + pad,), -7.25, dtype=torch.float64, device=device), torch.full((B + pad,), -7, dtype=torch.int32, device=device)

    ll, lp, st = buffers()
    case.ctx.eval_batch(theta, loglike=ll[:B], logprior=lp[:B], status=st[:B])
    post, stp = buffers()[::2]
    case.ctx.eval_logposterior(theta, post[:B], status=stp[:B])
    torch.cuda.synchronize(device)
    host = evaluate(case, B)
    for got, ref in zip((ll, lp, st, post, stp), host):
        assert same_bits(got[:B].cpu().numpy(), ref), (case.name, B)
        assert (got[B:] == (-7 if got.dtype == torch.int32 else -7.25)).all(), (case.name, B)
    for keep in range(3):
        out = buffers()
        case.ctx.eval_batch(theta, **{key: tensor[:B] for k, (key, tensor) in enumerate(zip(['loglike', 'logprior', 'status'], out)) if k == keep})
        torch.cuda.synchronize(device)
        assert same_bits(out[keep][:B].cpu().numpy(), host[keep]), (case.name, B, keep)
        for k in range(3): assert (out[k][B:] == (-7 if k == 2 else -7.25)).all() and (k == keep or (out[k] == (-7 if k == 2 else -7.25)).all())
    post = buffers()[0]
    case.ctx.eval_logposterior(theta, post[:B], status=None)
    torch.cuda.synchronize(device)
    assert same_bits(post[:B].cpu().numpy(), host[3]) and (post[B:] == -7.25).all()


@pytest.mark.parametrize('name', ['p1', 'p6', 'p8', 'p9', 'p15', 'p26'])
def test_record_against_the_finalize_that_evaluates_the_priors(name):
    case = Case.get(name)
    for B in BATCHES: check_batch(case, B)


@pytest.mark.parametrize('name', ['p6', 'p9', 'p26'])
def test_outputs_beyond_the_batch_and_null_output_pointers(name):
    case = Case.get(name)
    for B in (1, 33, 65, 257): check_device_outputs(case, B)


def test_two_observables_one_record_per_point():
    case = Case.get('two')
    for B in (32, 33): check_batch(case, B, 'merged launch')
    with switches(DL_NO_MERGED_THEORY='1'):
        for B in (32, 33): check_batch(case, B, 'one launch per observable')
    check_device_outputs(case, 32)


@pytest.mark.parametrize('env', [dict(DL_CG_MT='16'), dict(DL_CG_MT='32'), dict(DL_CHI2_FUSED='1'), dict(DL_STEP_KERNEL='1')], ids=lambda env: '-'.join(env))
def test_forced_tiles_and_fused_forms_against_the_default(env):
    # (dl_step_kernel runs the theory on its interval-polynomial path, which agrees with the moment form to rounding only: both sides of its comparison take that path)
    base = dict(DL_FS_NO_MOMENTS='1') if 'DL_STEP_KERNEL' in env else {}
    for name, batches in [('p6', (33, 256, 257)), ('p9', (65, 256))]:
        case = Case.get(name)
        for B in batches:
            with switches(**base):
                default = evaluate(case, B)
                with switches(**env):
                    forced = evaluate(case, B)
                    check_batch(case, B, '-'.join(env))       # (with the switch set: the record against the finalize that evaluates the priors)
            for got, ref in zip(forced, default): assert same_bits(got, ref), (name, B, env)


@pytest.mark.parametrize('env', [dict(DL_FS_WIDE='0', DL_FS_DENSE_MIN='256'), dict(DL_NO_TOEPLITZ='1')], ids=lambda env: '-'.join(env))
def test_other_theory_kernels_in_a_child_process(env):
    """Switches read once per process: the 256-thread form at every batch size and the DENSE form at 257 points; the generic kernel."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(out.stdout.decode()[-2000:])
    assert out.returncode == 0 and 'every case ok' in out.stdout.decode(), out.stderr.decode()[-2000:]


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    for name in ['p6', 'p15', 'two']:
        for B in ((32, 33) if name == 'two' else BATCHES): check_batch(Case.get(name), B)
    print('every case ok')
