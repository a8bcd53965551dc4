"""Shared pieces of the prior-box fixtures (tests/golden/make_priorbox_fixture.py, tests/test_priorbox_fixtures.py, tests/test_gpu_priorbox.py): which configurations
there are, the rule that gives the box from the priors, the row kinds, the hash that ties ``priorbox_<name>.npz`` to its companion ``boundary_<name>.npz``.
Test infrastructure only: numpy and the standard library."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

# name -> (rows, parameters whose corners are enumerated); the companion is boundary_<name>.npz.  No reference evaluation here is slow (the slowest, one-loop TNS, takes
# 0.2 s): every plain configuration gets the full 64 rows with 32 corners
PLAIN = {name: (64, 5) for name in ['cfg2_dense', 'two_tracers', 'eft_qisoqap',
                                    'cfg4_pk', 'cfg4_xi', 'cfg4_resummed', 'cfg4_resummed_xi_binned', 'cfg4_flexible', 'cfg4_models', 'cfg4_pk_pcs', 'cfg4_xi_pcs2',
                                    'kaiser_xi', 'xi_binned', 'tns', 'tns_eft', 'png', 'png_velocity', 'turnover', 'bands', 'phaseshift_pk', 'phaseshift_xi',
                                    'cfg3', 'cfg3_taylor', 'cfg3_taylor_standard', 'cfg3_stacked', 'cfg3_stacked_lpt']}
SOLVED = {'cfg4_xi_marg': (16, 3), 'two_tracers_marg': (16, 3)}
FIXTURES = dict(PLAIN, **SOLVED)
# every fixture whose observables go through the full-shape theory kernels on uniform template knots (theory 0 / 1 on the ShapeFit, turn-over or band template; xi through
# the folded Hankel window; a solved two-tracer context): what DL_FS_NO_MOMENTS, DL_NO_TOEPLITZ and DL_FS_WIDE switch.  The one-loop and PNG kernels take the same
# convolution for their splines: DL_NO_TOEPLITZ switches them too (tests/test_gpu_switches.py)
FULLSHAPE = ['cfg2_dense', 'two_tracers', 'eft_qisoqap', 'kaiser_xi', 'xi_binned', 'turnover', 'bands', 'two_tracers_marg']
TOEPLITZ = FULLSHAPE + ['tns', 'tns_eft', 'png', 'png_velocity']

# Boxes that had to shrink: the lower prior limit is a pole of the reference's own theory, where it returns nan on more than 10 % of the rows.  'bands': the velocity
# bands enter as dptt / df^2, nan at df = 0 whatever the other parameters.  'turnover': the template has dpto^-n, nan at dpto = 0 unless n = 0.  The reference is finite on
# every point above the pole that was tried (from 1e-30 on) but grows as 1 / df^2 and dpto^-n towards it, so "the widest finite range" has no smallest end: the box starts
# 1e-3 of the prior range above the pole (log-likelihoods of -2e11 and -1e4 there), a choice made from the reference alone.  name -> {parameter: (lo, hi)}, None: kept
SHRUNK = {'bands': {'df': (2e-3, None)}, 'turnover': {'dpto': (2e-3, None)}}

KIND_CENTRE, KIND_CORNER, KIND_ALL, KIND_ONE, KIND_UNIFORM = range(5)
MAX_BYTES, MAX_TOTAL_BYTES, MAX_BAD = 400000, 6000000, 0.1


def companion_path(name):
    return os.path.join(GOLDEN, 'boundary_{}.npz'.format(name))


def priorbox_path(name):
    return os.path.join(GOLDEN, 'priorbox_{}.npz'.format(name))


def load_companion(name):
    """(archive as a dictionary, {dl_config key: array}) of ``boundary_<name>.npz``."""
    with np.load(companion_path(name)) as g:
        g = {key: g[key] for key in g.files}
    return g, {key[4:]: value for key, value in g.items() if key.startswith('cfg/')}


def load_priorbox(name):
    with np.load(priorbox_path(name)) as g:
        return {key: g[key] for key in g.files}


def cfg_sha(archive):
    """sha256 over the sorted ``cfg/`` keys of a companion archive: name, dtype, shape and bytes of each."""
    h = hashlib.sha256()
    for key in sorted(key for key in archive if key.startswith('cfg/')):
        value = np.ascontiguousarray(archive[key])
        h.update(key.encode()); h.update(value.dtype.str.encode()); h.update(repr(value.shape).encode()); h.update(value.tobytes())
    return h.hexdigest()


def finite_uniform(priors):
    """Which parameters have a uniform prior with two finite limits (rows (kind, lo, hi, loc, scale) of the key ``priors``)."""
    priors = np.asarray(priors, dtype='f8').reshape(-1, 5)
    return (priors[:, 0] == 0) & np.isfinite(priors[:, 1]) & np.isfinite(priors[:, 2])


def box_from_priors(priors, value=None, ref_width=None):
    """``box [P, 2]``: uniform prior -> its limits; normal prior -> loc +- 3 scale within its limits; a side without a finite limit of a flat prior -> the parameter's
    value -+ 5 widths of its start distribution (``value``, ``ref_width``: needed for those sides only; without them they come out as nan)."""
    priors = np.asarray(priors, dtype='f8').reshape(-1, 5)
    box = priors[:, 1:3].copy()
    normal = priors[:, 0] == 1
    assert np.isin(priors[:, 0], [0, 1]).all(), 'the rule covers uniform and normal priors'
    box[normal, 0] = np.maximum(box[normal, 0], priors[normal, 3] - 3. * priors[normal, 4])
    box[normal, 1] = np.minimum(box[normal, 1], priors[normal, 3] + 3. * priors[normal, 4])
    for side, sign in enumerate((-1., 1.)):
        open_side = ~np.isfinite(box[:, side])
        if open_side.any():
            box[open_side, side] = np.nan if value is None else (np.asarray(value, dtype='f8') + sign * 5. * np.asarray(ref_width, dtype='f8'))[open_side]
    return box


def shrink(name, names, box):
    """``box`` with the entries of ``SHRUNK[name]`` put in."""
    box = np.array(box, dtype='f8')
    for pname, sides in SHRUNK.get(name, {}).items():
        for side, value in enumerate(sides):
            if value is not None: box[list(names).index(pname), side] = value
    return box


def corner_columns(priors, ncorner):
    return np.flatnonzero(finite_uniform(priors))[:ncorner]


def rows_in_box(box, priors, size, ncorner, seed):
    """``(theta [size, P], row_kind [size])``: the centre; every corner over the first ``ncorner`` parameters with finite uniform limits (the others at the centre); all at lo,
    all at hi, lo / hi alternating; one parameter at a time at lo and at hi (at most 24 rows, in parameter order); the rest uniform over the box."""
    box = np.asarray(box, dtype='f8')
    npar = len(box)
    centre = 0.5 * (box[:, 0] + box[:, 1])
    rows, kinds = [centre.copy()], [KIND_CENTRE]
    cols = corner_columns(priors, ncorner)
    for icorner in range(2**len(cols)):
        row = centre.copy()
        for ibit, col in enumerate(cols): row[col] = box[col, (icorner >> ibit) & 1]
        rows.append(row); kinds.append(KIND_CORNER)
    rows += [box[:, 0].copy(), box[:, 1].copy(), box[np.arange(npar), np.arange(npar) % 2].copy()]; kinds += [KIND_ALL] * 3
    for ipar in range(npar):
        for side in range(2):
            if len(rows) >= size or kinds.count(KIND_ONE) >= 24: break
            row = centre.copy(); row[ipar] = box[ipar, side]
            rows.append(row); kinds.append(KIND_ONE)
    rng = np.random.RandomState(seed)
    while len(rows) < size:
        rows.append(rng.uniform(box[:, 0], box[:, 1])); kinds.append(KIND_UNIFORM)
    assert len(rows) == size, (len(rows), size)
    return np.array(rows), np.array(kinds, dtype='i4')


def marginalised_logposterior(c, g, H, marg):
    """The closed form from the exact quadratic (c, g, H) of the unsolved log-posterior in the solved parameters (likelihoods/base.py:385-404 of the reference: no 2 pi):
    ``(logposterior, dx)`` with the solved parameters at ``x0 + dx``; ``marg``: which of them are marginalised ('.marg': their determinant counts) and not profiled."""
    dx = -np.linalg.solve(H, g)
    marg = np.asarray(marg).astype(bool)
    return c + 0.5 * g.dot(dx) - (0.5 * np.linalg.slogdet(-H[np.ix_(marg, marg)])[1] if marg.any() else 0.), dx


def shotnoise_rounding(cfg):
    """``4 eps max|shotnoise_out|``: the reference forms ``W (P + shotnoise_in) - shotnoise_out``, so no entry of its theory vector is better than a rounding at the size of
    ``shotnoise_out``, whatever is left after the subtraction.  Measured against a long-double evaluation of that expression (docs/EXPERIMENTS.md): the reference is off by
    up to 6.5e-13 on 'cfg4_resummed' (shot noise 3e3, eps 3e3 = 6.7e-13; its corners leave a theory vector of 0.88 and less) and by 1.8e-12 at row 9 of 'two_tracers_marg'
    (shot noise 1e4; every bias and the growth rate at 0: exact value 0).  Four times the rounding is the factor the project grants a measured rounding error."""
    shotnoise = [np.abs(value).max() for key, value in cfg.items() if key.endswith('.shotnoise_out') and np.size(value)]
    return 4. * np.finfo('f8').eps * max(shotnoise, default=0.)


def flattheory_error(flat, ref_flat, cfg):
    """Largest error of the theory vectors ``flat [N, n]`` against the reference's, per row, over the row's bound: 1e-10 of the row's largest reference magnitude plus
    ``shotnoise_rounding(cfg)``, which decides only where the theory all but vanishes.  Without shot-noise keys the bound is the first term alone: a zero row must be zero."""
    bound = 1e-10 * np.abs(ref_flat).max(axis=1) + shotnoise_rounding(cfg)
    error = np.abs(flat - ref_flat).max(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(error == 0., 0., error / bound)      # (a zero bound is met by a zero error only)
    return np.where(np.isfinite(ratio), ratio, np.inf)
