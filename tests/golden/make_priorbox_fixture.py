"""The reference over the whole prior box (build container only; the reference never travels to the GPU box):

    python tests/golden/make_priorbox_fixture.py [name ...]

The other generators of this directory draw their points from ``Parameter.ref``, the narrow start distribution of a sampler: a few per cent of the prior range around the
fiducial point.  This one evaluates the SAME reference likelihoods -- built by the same code: the builders of make_boundary_fixture.py, make_tns_fixture.py,
make_png_fixture.py, make_png_velocity_fixture.py, make_turnover_fixture.py, make_bands_fixture.py and make_phaseshift_fixture.py are run with their ``dump`` replaced by
the one below, so every likelihood is constructed by the lines that constructed the companion ``boundary_<name>.npz`` -- at the centre, the corners, the faces and uniform
points of the box the priors span (tests/priorbox_utils.py::box_from_priors, rows_in_box) and stores in ``priorbox_<name>.npz``, data only:

    names, theta [N, P], box [P, 2], row_kind [N], row_bad [N], loglikelihood, logprior, logposterior [N], flattheory [N, n], cfg_sha,
    value [P], ref_width [P] (the parameters' values; the widths of their start distributions where a flat prior has an open side, which the box rule needs; nan elsewhere)

``cfg_sha`` (priorbox_utils.cfg_sha) ties the file to the constants of its companion, which it does not repeat.  ``row_bad``: rows on which the reference raised or returned
a non-finite value (stored as nan); ``box`` is the rule's unless priorbox_utils.SHRUNK says otherwise (a pole of the reference on a prior limit).  Configurations with analytically solved parameters: the reference's ``_solve`` needs jax, so -- as make_boundary_fixture.py::dump does
-- the unsolved pipeline gives the exact quadratic form ``marg_c, marg_g, marg_H`` at ``marg_x0`` on every row; ``logposterior`` is the closed form of it,
``loglikelihood`` / ``logprior`` / ``flattheory`` are the unsolved pipeline's at ``marg_x0``.

Child processes, one family of builders each (the one-loop fixtures scale the stand-in cosmology through the environment, some families patch a helper of the
reference for numpy), four at a time.  The archives are written with fixed time stamps and sorted keys: a second run gives the same bytes.
"""
import os
import subprocess
import sys
import time
import warnings

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
sys.path.insert(0, here)
sys.path.insert(0, os.path.join(root, 'tests'))
warnings.filterwarnings('ignore')

import priorbox_utils as pbu   # noqa: E402

SELECTED = set()


def ref_width(param):
    """Width of the start distribution: the scale of a normal one, half the range of a uniform one."""
    ref = param.ref
    if ref.dist == 'norm': return float(ref.attrs['scale'])
    lo, hi = ref.limits
    assert np.isfinite([lo, hi]).all(), 'no width for the start distribution of {}'.format(param.name)
    return 0.5 * (float(hi) - float(lo))


def evaluate(likelihood, names, row):
    """(loglikelihood, logprior, logposterior, flattheory) of the reference at one point; None where it raises or returns a non-finite value."""
    try:
        logposterior = float(likelihood(**dict(zip(names, row))))
        out = float(np.ravel(likelihood.loglikelihood)[0]), float(np.ravel(likelihood.logprior)[0]), logposterior, np.array(likelihood.flattheory, dtype='f8')
    except Exception as exc:
        print('    reference raised at', dict(zip(names, row)), repr(exc)[:200])
        return None
    return out if np.isfinite(out[:3]).all() and np.isfinite(out[3]).all() else None


EMITTED = []


def emit(name, likelihood, size=None, seed=42, unsolved=None, extras=None):
    """Stands in for ``make_boundary_fixture.dump``: same arguments, writes ``priorbox_<name>.npz``."""
    if name not in pbu.FIXTURES or (SELECTED and name not in SELECTED): return
    EMITTED.append(name)
    import make_boundary_fixture as mb
    from make_phaseshift_fixture import savez_reproducible
    t0 = time.time()
    if not hasattr(likelihood, 'all_params'): likelihood = likelihood()
    if unsolved is not None and not hasattr(unsolved, 'all_params'): unsolved = unsolved()
    try:
        likelihood()
    except (ModuleNotFoundError, AttributeError) as exc:   # the analytic solve needs jax; the pipeline has been initialised by then
        assert 'jax' in str(exc) and unsolved is not None
    companion, cfg = pbu.load_companion(name)
    names = [str(n) for n in companion['names']]
    params = [likelihood.varied_params[n] for n in names]
    assert len(params) == len(likelihood.varied_params)
    priors = cfg['priors'].reshape(-1, 5)
    need = ~np.isfinite(priors[:, 1:3]).all(axis=1) & (priors[:, 0] == 0)
    value, width = np.array([float(param.value) for param in params]), np.array([ref_width(param) if flag else np.nan for param, flag in zip(params, need)])
    box = pbu.box_from_priors(priors, value=value, ref_width=width)
    box = pbu.shrink(name, names, box)
    nrows, ncorner = pbu.FIXTURES[name]
    theta, row_kind = pbu.rows_in_box(box, priors, nrows, ncorner, seed + 1000)
    out = dict(names=np.array(names), theta=theta, box=box, row_kind=row_kind, cfg_sha=np.array(pbu.cfg_sha(companion)), value=value, ref_width=width)
    model, columns = likelihood, names
    if name in pbu.SOLVED:
        solved = [str(n) for n in companion['solved']]
        unsolved()
        x0 = np.array([likelihood.all_params[n].value for n in solved])
        assert np.array_equal(x0, companion['marg_x0'])
        model, columns = unsolved, names + solved
        theta = np.column_stack([theta, np.tile(x0, (nrows, 1))])
    rows = [evaluate(model, columns, row) for row in theta]
    row_bad = np.array([row is None for row in rows])
    ndata = max(row[3].size for row in rows if row is not None)
    for ikey, key in enumerate(['loglikelihood', 'logprior', 'logposterior']): out[key] = np.array([np.nan if row is None else row[ikey] for row in rows])
    out['flattheory'] = np.array([np.full(ndata, np.nan) if row is None else row[3] for row in rows])
    if name in pbu.SOLVED:
        ns = len(solved)
        quad = []
        for irow, row in enumerate(out['theta']):
            base = dict(zip(names, row))
            try:
                if row_bad[irow]: raise FloatingPointError('row is bad already')
                quad.append(mb.exact_quadratic(lambda x: unsolved(**{**base, **dict(zip(solved, x))}), x0))
            except (AssertionError, FloatingPointError) as exc:
                print('    no exact quadratic at row', irow, repr(exc)[:200])
                row_bad[irow] = True
                quad.append((np.nan, np.full(ns, np.nan), np.full((ns, ns), np.nan)))
        out.update(solved=np.array(solved), marg_x0=x0, marg_c=np.array([q[0] for q in quad]), marg_g=np.array([q[1] for q in quad]), marg_H=np.array([q[2] for q in quad]))
        out['logposterior'] = np.array([np.nan if bad else pbu.marginalised_logposterior(c, g, H, cfg['marg.kind'])[0] for bad, c, g, H in zip(row_bad, out['marg_c'], out['marg_g'], out['marg_H'])])
    out['row_bad'] = row_bad
    fn = pbu.priorbox_path(name)
    savez_reproducible(fn, out)
    print('saved {} {:.1f} kB, {:d} rows, {:d} bad, {:.1f} s'.format(os.path.basename(fn), os.path.getsize(fn) / 1e3, nrows, int(row_bad.sum()), time.time() - t0), flush=True)
    assert os.path.getsize(fn) <= pbu.MAX_BYTES and row_bad.mean() <= pbu.MAX_BAD, 'more than 10 % of the rows of {} are not finite: find the parameter and shrink its box (tests/priorbox_utils.py::SHRUNK)'.format(name)


# what each family of builders must hand over: a builder that stops calling ``make_boundary_fixture.dump`` by that name (bound at import, renamed, dropped) fails the run
# instead of silently leaving a fixture out
FAMILY_FIXTURES = {'tns': ['tns', 'tns_eft'], 'png': ['png'], 'png_velocity': ['png_velocity'], 'turnover': ['turnover'], 'bands': ['bands'], 'phaseshift': ['phaseshift_pk', 'phaseshift_xi']}
FAMILY_FIXTURES['boundary'] = [name for name in pbu.FIXTURES if name not in sum(FAMILY_FIXTURES.values(), [])]


def run_family(family):
    try:
        _run_family(family)
    finally:
        expected = [name for name in FAMILY_FIXTURES[family] if not SELECTED or name in SELECTED]
        assert sorted(EMITTED) == sorted(expected), 'family {}: expected {}, the builders handed over {}'.format(family, expected, EMITTED)


def _run_family(family):
    import make_boundary_fixture as mb
    mb.dump = emit          # every builder below hands its likelihood to ``mb.dump``
    if family == 'boundary':
        mb.main()
    elif family == 'phaseshift':
        import make_phaseshift_fixture as mp
        from cosmoprimo.cosmology import SyntheticPk

        def emit_phaseshift(name, build, klim=(1e-5, 1e2), seed=42):
            SyntheticPk.extrap_kmin, SyntheticPk.extrap_kmax = klim     # (as make_phaseshift_fixture.dump sets them)
            emit('phaseshift_' + name, build, seed=seed)

        mp.dump = emit_phaseshift
        mp.main()
    else:
        __import__('make_{}_fixture'.format(family)).boundary()


# the families, the largest split so that the children take about as long as each other (None: whatever fixtures the family has)
TASKS = [('boundary', ['cfg3', 'cfg3_taylor', 'cfg3_taylor_standard']), ('boundary', ['cfg3_stacked', 'cfg3_stacked_lpt']), ('tns', None),
         ('boundary', ['cfg2_dense', 'two_tracers', 'eft_qisoqap', 'kaiser_xi', 'xi_binned', 'two_tracers_marg']),
         ('boundary', ['cfg4_pk', 'cfg4_xi', 'cfg4_resummed', 'cfg4_resummed_xi_binned', 'cfg4_flexible', 'cfg4_models', 'cfg4_pk_pcs', 'cfg4_xi_pcs2', 'cfg4_xi_marg']),
         ('phaseshift', None), ('png', None), ('png_velocity', None), ('turnover', None), ('bands', None)]


def main():
    argv = sys.argv[1:]
    family = None
    if '--family' in argv:
        family = argv[argv.index('--family') + 1]
        del argv[argv.index('--family'):argv.index('--family') + 2]
    unknown = set(argv) - set(pbu.FIXTURES)
    assert not unknown, unknown
    SELECTED.update(argv)
    if family is not None: return run_family(family)
    assert sorted(sum([names for _, names in TASKS if names], [])) == sorted(FAMILY_FIXTURES['boundary'])
    t0 = time.time()
    running, failed = [], []
    pending = list(TASKS)
    while pending or running:       # four children at a time
        while pending and len(running) < 4:
            family, names = pending.pop(0)
            if names is not None and SELECTED: names = [name for name in names if name in SELECTED]
            if names is not None and not names: continue
            running.append((family, subprocess.Popen([sys.executable, os.path.abspath(__file__), '--family', family] + list(names if names is not None else SELECTED))))
        time.sleep(0.5)
        for item in list(running):
            if item[1].poll() is not None:
                running.remove(item)
                if item[1].returncode != 0: failed.append(item[0])
    assert not failed, failed
    print('done in {:.0f} s'.format(time.time() - t0))


if __name__ == '__main__':
    main()
