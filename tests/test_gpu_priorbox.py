"""GPU (-m gpu): every theory against the REFERENCE over its whole prior box.

``tests/golden/priorbox_<name>.npz`` (tests/golden/make_priorbox_fixture.py) hold the reference's own log-likelihood, log-prior and theory vector at the centre, the
corners, the faces and uniform points of the box the priors span -- where the other fixtures, drawn from the samplers' start distribution, cover a few per cent of it
around the fiducial point.  The contexts are created from the keys of the companion ``boundary_<name>.npz`` alone, as tests/test_gpu_boundary.py does.

Bounds (the project's standing ones, none derived from the device): ``|logL - ref| <= 1e-10 max(1, |ref|)``; log-prior at 1e-13; the theory vector within 1e-10 of the
row's largest reference magnitude (plus four roundings of the reference's own shot-noise subtraction: priorbox_utils.flattheory_error); solved parameters: the closed form of the reference's exact quadratic, 1e-10 (tests/test_gpu_boundary.py).  The same rows through
the other launches: one point; 257 points (past the 256-point switch of the theory kernel's form); 2100 points (past the 2048-row switch from the chi2 GEMM to the
large-batch routes); every configuration on the full-shape theory kernels (priorbox_utils.FULLSHAPE) with the interval polynomials (``DL_FS_NO_MOMENTS=1``) and, in a child process each (read once per process),
without the Toeplitz convolution (``DL_NO_TOEPLITZ=1``: also the one-loop and PNG kernels) and on the 256-thread form (``DL_FS_WIDE=0``).  Every check prints its figures by row kind before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path[:0] = [d for d in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))) if d not in sys.path]   # (the child process is started as a script)

import priorbox_utils as pbu

pytestmark = pytest.mark.gpu

KIND_NAMES = ['centre', 'corner', 'all', 'one', 'uniform']
_loaded, _context = {}, {}


def load(name):
    if name not in _loaded:
        companion, cfg = pbu.load_companion(name)
        g = pbu.load_priorbox(name)
        assert str(g['cfg_sha']) == pbu.cfg_sha(companion)
        _loaded[name] = (g, cfg)
    return _loaded[name]


def context(name):
    """The context of ``name`` from the companion's keys; one is alive at a time."""
    if name not in _context:
        from desilike_amd._lib import Context
        _context.clear()
        _context[name] = Context(load(name)[1], device=0)
    return _context[name]


def by_kind(error, kinds):
    return ', '.join('{} {:.1e}'.format(KIND_NAMES[kind], np.nanmax(error[kinds == kind])) for kind in np.unique(kinds))


def measure(name, rows, batch=None):
    """The fixture rows ``rows`` of ``name``, evaluated as the first rows of a call of ``batch`` points (the fixture rows cycled; default: just them): the device's outputs
    and their errors against the reference, per row.  ``logl``: |logL - ref| / max(1, |ref|) (solved parameters: of the marginalised log-posterior); ``flat``: largest
    error of the theory vector over the row's bound (priorbox_utils.flattheory_error), in units of 1e-10; ``prior``: |logprior - ref| / max(1, |ref|); ``solved``: error of the solved parameters over
    the bound rtol 1e-7, atol 1e-9 max|x| of tests/test_gpu_boundary.py."""
    g, cfg = load(name)
    ctx = context(name)
    rows = np.asarray(rows)
    index = rows if batch is None else np.concatenate([rows, np.arange(batch - len(rows)) % len(g['theta'])])
    solved = name in pbu.SOLVED
    out = ctx.eval_batch_host(g['theta'][index], return_flattheory=True, return_solved=solved)
    loglike, logprior, status, flat = (a[:len(rows)] for a in out[:4])
    ref_flat = g['flattheory'][rows]
    m = dict(n=len(index), rows=rows, bad=g['row_bad'][rows], kinds=g['row_kind'][rows], loglike=loglike, status=status, flattheory=flat)
    m['flat'] = pbu.flattheory_error(flat, ref_flat, cfg)
    if solved:
        ref = g['logposterior'][rows]
        m['logl'] = np.abs(loglike + logprior - ref) / np.maximum(1., np.abs(ref))
        m['prior'] = np.zeros(len(rows))       # (the closed form gives the sum only)
        x = np.array([g['marg_x0'] + pbu.marginalised_logposterior(g['marg_c'][row], g['marg_g'][row], g['marg_H'][row], cfg['marg.kind'])[1] for row in rows])
        m['solved'] = (np.abs(out[4][:len(rows)] - x) / (1e-7 * np.abs(x) + 1e-9 * np.abs(x).max(axis=1)[:, None])).max(axis=1)
    else:
        ref = g['loglikelihood'][rows]
        m['logl'] = np.abs(loglike - ref) / np.maximum(1., np.abs(ref))
        m['prior'] = np.abs(logprior - g['logprior'][rows]) / np.maximum(1., np.abs(g['logprior'][rows]))
        m['solved'] = np.zeros(len(rows))
    return m


def check(name, rows, batch=None, label=''):
    m = measure(name, rows, batch=batch)
    good, bad = ~m['bad'], m['bad']
    print('{} {}B={:d}: logL error / max(1, |logL|) by row kind: {}; theory error / bound: {}'.format(name, label, m['n'], by_kind(m['logl'], m['kinds']), by_kind(m['flat'], m['kinds'])))
    assert (m['status'][good] == 0).all(), (name, m['rows'][m['status'] != 0])
    assert not (np.isfinite(m['loglike'][bad]) & (m['status'][bad] == 0)).any()            # where the reference has no finite value the device must not offer one
    for key, bound in [('logl', 1e-10), ('flat', 1.), ('prior', 1e-13), ('solved', 1.)]:
        assert (m[key][good] <= bound).all(), (name, key, 'row', m['rows'][good][np.argmax(m[key][good])], float(m[key][good].max()))
    return m['flattheory']


def corner_rows(g, n=4):
    """``n`` corner rows spread over the corners (first, last and between)."""
    corners = np.flatnonzero(g['row_kind'] == pbu.KIND_CORNER)
    return corners[np.linspace(0, len(corners) - 1, n).astype(int)]


@pytest.mark.parametrize('name', list(pbu.FIXTURES))
def test_prior_box_vs_reference(name):
    g, cfg = load(name)
    check(name, np.arange(len(g['theta'])))


@pytest.mark.parametrize('name', list(pbu.FIXTURES))
def test_prior_box_in_other_launches(name):
    g, cfg = load(name)
    every = np.arange(len(g['theta']))
    for row in corner_rows(g): check(name, [row])
    check(name, every, batch=257)
    check(name, every, batch=2100)


SWITCHED = {'DL_FS_NO_MOMENTS=1': pbu.FULLSHAPE, 'DL_NO_TOEPLITZ=1': pbu.TOEPLITZ, 'DL_FS_WIDE=0': pbu.FULLSHAPE}    # switch -> the fixtures whose kernels read it
_default = {}


def run_switched(names, label=''):
    """{name: sha256 of the theory vectors} of ``names`` at N points, 257 points and one corner, every launch checked against the reference."""
    import hashlib
    digests = {}
    for name in names:
        g, cfg = load(name)
        every = np.arange(len(g['theta']))
        flats = [check(name, every, label=label), check(name, every, batch=257, label=label), check(name, corner_rows(g)[:1], label=label)]
        digests[name] = hashlib.sha256(b''.join(np.ascontiguousarray(flat).tobytes() for flat in flats)).hexdigest()
    return digests


def default_digests(names):
    """The same launches with no switch set, run once per fixture in this process."""
    _default.update(run_switched([name for name in names if name not in _default]))
    return {name: _default[name] for name in names}


def test_interval_polynomial_form():
    """``DL_FS_NO_MOMENTS=1``: the spline from interval polynomials instead of (knot value, moment) records -- other end corrections, other extrapolation code."""
    from desilike_amd._lib import refresh_options
    names = SWITCHED['DL_FS_NO_MOMENTS=1']
    default = default_digests(names)
    os.environ['DL_FS_NO_MOMENTS'] = '1'; refresh_options()
    try:
        polynomial = run_switched(names, 'DL_FS_NO_MOMENTS=1 ')
    finally:
        del os.environ['DL_FS_NO_MOMENTS']; refresh_options()
    switched = [name for name in names if default[name] != polynomial[name]]
    print('the switch changed the bits of', switched)
    assert switched            # (it did select another path)


@pytest.mark.parametrize('switch', ['DL_NO_TOEPLITZ=1', 'DL_FS_WIDE=0'])
def test_theory_forms_in_a_child_process(switch):
    """Read once per process: the child runs every fixture whose kernels read the switch, checks each against the reference and prints a digest of its theory vectors;
    the digests of this process's own run without the switch show that another path ran."""
    key, value = switch.split('=')
    names = SWITCHED[switch]
    default = default_digests(names)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), switch], env=dict(os.environ, **{key: value}), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    stdout = out.stdout.decode()
    print(stdout[-6000:])
    assert out.returncode == 0 and 'every case ok' in stdout, out.stderr.decode()[-3000:]
    child = dict(line.split()[1:3] for line in stdout.splitlines() if line.startswith('digest '))
    assert sorted(child) == sorted(names)
    switched = [name for name in names if child[name] != default[name]]
    print('the switch changed the bits of', switched)
    # The 512- and the 256-thread form do the same arithmetic per wavenumber in another thread layout: their theory vectors agree bit for bit on every fixture (measured: all
    # eight digests equal), so no output can witness DL_FS_WIDE; what stands for it is the child's environment (asserted there) and dl_kernels.hip reading it per process.
    if switch != 'DL_FS_WIDE=0': assert switched


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    key, value = sys.argv[1].split('=')
    assert os.environ.get(key) == value
    for name, digest in run_switched(SWITCHED[sys.argv[1]], sys.argv[1] + ' ').items(): print('digest', name, digest)
    print('every case ok')
