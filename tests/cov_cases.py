"""Cases for the covariance plan (``CovariancePlanBuilder``, csrc/dl_cov.hip) beyond the three fixtures of tests/golden/covariance.npz: synthetic observables, as the
dicts ``orc.gaussian_covariance`` takes, on deliberately different theory grids.  No device library here: tests/test_cov_cases.py checks builder + plan interpreter
(tests/cov_plan_numpy.py) against the oracle on the CPU, tests/test_gpu_cov_shapes.py runs the kernel.

Spectra: a power law times a damped wiggle, times (1 + 1 % noise), positive, one amplitude per multipole; ``B = 3`` draws per case."""
import collections

import numpy as np

B = 3
AMPLITUDE = {0: 2e4, 2: 1e4, 4: 3e3, 6: 8e2, 8: 2e2}

# the project's tolerance for this kernel (tests/test_covariance.py)
RTOL, ATOL = 1e-11, 1e-13


def lin(lo, hi, n): return np.linspace(lo, hi, n)


def geo(lo, hi, n): return np.geomspace(lo, hi, n)


def bins(edges):
    edges = np.asarray(edges, dtype='f8')
    return np.column_stack([edges[:-1], edges[1:]])


def pk(ells, edges, theory_k, theory_ells, volume=2e9, shotnoise=4e3):
    return dict(kind='pk', ells=tuple(ells), edges=[np.asarray(e, dtype='f8') for e in edges], volume=volume, shotnoise=shotnoise, theory_k=theory_k, theory_ells=tuple(theory_ells))


def xi(ells, edges, theory_k, theory_ells, volume=2e9, shotnoise=4e3):
    return dict(pk(ells, edges, theory_k, theory_ells, volume=volume, shotnoise=shotnoise), kind='xi')


def _cases():
    cases = collections.OrderedDict()
    # theories without monopole (ell0 = -1): no shot noise anywhere in sigma, no zero lag to remove in xi x xi; P listed before xi: the transposed cross block
    cases['no_monopole'] = dict(resolution=1, reaches=('ell0_none', 'pk_before_xi'), observables=[
        pk((2, 4), [bins(lin(0.02, 0.2, 10))] * 2, lin(0.01, 0.25, 30), (2, 4)),
        xi((2,), [bins(lin(20., 120., 6))], geo(0.002, 0.6, 36), (2, 4), shotnoise=2.5e3)])
    # five theory multipoles (DL_COV_MAX_ELLS), five integration points
    cases['five_ells'] = dict(resolution=5, reaches=('n_ell_5',), observables=[
        pk((0, 2, 4), [bins(lin(0.01, 0.15, 8)), bins(lin(0.01, 0.15, 8)), bins(lin(0.03, 0.12, 4))], geo(0.005, 0.3, 33), (0, 2, 4, 6, 8))])
    # two P observables, bin widths 0.02 and 0.05 / 0.045 with offsets: partial and empty intersections, [0.04, 0.06] inside [0.025, 0.075]; bins below and above the
    # k range of both theories ([0.035, 0.17] and [0.03, 0.16]); a multipole with one bin
    cases['two_pk'] = dict(resolution=2, reaches=('partial_intersections', 'clipping', 'one_bin'), observables=[
        pk((0, 2), [bins(lin(0.02, 0.2, 10)), bins(lin(0.02, 0.2, 10))[2:7]], lin(0.035, 0.17, 25), (0, 2, 4), volume=3e9),
        pk((0, 2, 4), [bins(lin(0.025, 0.225, 5)), bins([0.06, 0.15]), bins(lin(0.01, 0.19, 5))], geo(0.03, 0.16, 19), (0, 2, 4), volume=2e9, shotnoise=1.5e3)])
    # xi, P, xi: P before xi (transposed) and xi before P (not transposed) in one plan; two xi observables on different k grids (the union grid, j1 != j2), s-bins
    # that overlap (const != 0) and that do not
    cases['xi_pk_xi'] = dict(resolution=2, reaches=('xi_before_pk', 'pk_before_xi', 'xi_xi_two_grids', 'const'), observables=[
        xi((0, 2), [bins(lin(20., 100., 5)), bins(lin(40., 100., 4))], geo(0.003, 0.5, 28), (0, 2, 4), shotnoise=3e3),
        pk((0, 2), [bins(lin(0.02, 0.14, 7)), bins(lin(0.02, 0.1, 5))], lin(0.01, 0.2, 21), (0, 2, 4), shotnoise=3e3),
        xi((0, 4), [bins([30., 55., 70., 130.]), bins([90., 150.])], lin(0.004, 0.45, 31), (0, 2, 4), volume=1.5e9, shotnoise=5e3)])
    # three observables mixing the above: xi(0, 2) + P(2, 4) without monopole + P(0) on five multipoles, three theory grids
    cases['three_mixed'] = dict(resolution=2, reaches=('ell0_none', 'n_ell_5', 'xi_before_pk', 'clipping'), observables=[
        xi((0, 2), [bins(lin(25., 125., 6)), bins(lin(25., 125., 6))[1:4]], geo(0.002, 0.4, 32), (0, 2, 4), shotnoise=2e3),
        pk((2, 4), [bins(lin(0.03, 0.21, 7)), bins(lin(0.05, 0.17, 4))], lin(0.04, 0.18, 23), (2, 4), volume=2.5e9),
        pk((0,), [bins(lin(0.015, 0.195, 10))], geo(0.01, 0.3, 27), (0, 2, 4, 6, 8), shotnoise=1e3)])
    # eight observables (DL_COV_MAX_THEORIES) with one to three bins each
    grids = [lin(0.01, 0.3, 12), geo(0.004, 0.4, 17), lin(0.02, 0.25, 9), geo(0.003, 0.5, 21)]
    cases['eight'] = dict(resolution=1, reaches=('eight_observables',), observables=[
        pk((0,), [bins([0.03, 0.06, 0.1])], grids[0], (0, 2)),
        xi((0,), [bins([30., 60.])], grids[1], (0, 2, 4)),
        pk((2,), [bins([0.05, 0.12])], grids[2], (2,), shotnoise=2e3),
        xi((2, 0), [bins([40., 80.]), bins([50., 70., 90.])], grids[3], (0, 2), volume=1e9),
        pk((0, 2), [bins([0.02, 0.07]), bins([0.04, 0.09, 0.11, 0.2])], grids[1], (0, 2, 4, 6, 8), shotnoise=6e3),
        xi((4,), [bins([25., 45.])], grids[0], (0, 4)),
        pk((4,), [bins([0.01, 0.3])], grids[3], (0, 2, 4)),
        xi((0,), [bins([55., 65.])], grids[2], (0,), shotnoise=1e3)])
    # a handful of cells: far fewer than one workgroup of 256
    cases['tiny'] = dict(resolution=1, reaches=('under_256_cells',), observables=[pk((0,), [bins([0.02, 0.05, 0.1, 0.11])], lin(0.01, 0.2, 5), (0,))])
    return cases


CASES = _cases()


def names():
    return list(CASES)


def spectra(name):
    """Per theory: power [B, n_ell, n_k], seeded by the case's position in the table."""
    rng = np.random.RandomState(700 + names().index(name))
    out = []
    for obs in CASES[name]['observables']:
        k = np.asarray(obs['theory_k'], dtype='f8')
        shape = (k / 0.1)**-1.2 * (1. + 0.15 * np.sin(k / 0.012) * np.exp(-(k / 0.25)**2))
        amp = np.array([AMPLITUDE[ell] for ell in obs['theory_ells']])
        tilt = rng.uniform(0.8, 1.25, size=(B, len(amp), 1))
        out.append(tilt * amp[None, :, None] * shape[None, None, :] * (1. + 0.01 * rng.standard_normal((B, len(amp), k.size))))
    return out


def oracle_inputs(name, ipoint):
    """(observables, theories, resolution) for ``orc.gaussian_covariance`` at draw ``ipoint``."""
    case = CASES[name]
    theories = [dict(k=obs['theory_k'], ells=list(obs['theory_ells']), power=power[ipoint]) for obs, power in zip(case['observables'], spectra(name))]
    return case['observables'], theories, case['resolution']


def plan_arguments(name):
    """What ``_lib.CovariancePlan`` takes, as ``ObservablesCovarianceMatrix._get_plan`` derives it: (arrays, n_ell, n_k, ell0, shotnoise)."""
    from desilike_amd.observables.galaxy_clustering.covariance import CovariancePlanBuilder
    case = CASES[name]
    desc = case['observables']
    arrays = CovariancePlanBuilder(desc, resolution=case['resolution']).arrays()
    n_ell, n_k = [len(d['theory_ells']) for d in desc], [len(d['theory_k']) for d in desc]
    ell0 = [list(d['theory_ells']).index(0) if 0 in d['theory_ells'] else -1 for d in desc]
    return arrays, n_ell, n_k, ell0, [d['shotnoise'] for d in desc]


_reference = {}


def reference(name):
    """``orc.gaussian_covariance`` at the B draws of the case [B, n, n]: computed once per process, read-only."""
    if name not in _reference:
        from oracle import np_oracle as orc
        ref = np.array([orc.gaussian_covariance(*oracle_inputs(name, ipoint)[:2], resolution=CASES[name]['resolution']) for ipoint in range(B)])
        ref.setflags(write=False)
        _reference[name] = ref
    return _reference[name]


def block_slices(name):
    sizes = [sum(len(e) for e in obs['edges']) for obs in CASES[name]['observables']]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    return [slice(int(lo), int(hi)) for lo, hi in zip(offsets[:-1], offsets[1:])]


def tolerance(name, ref):
    """The project's bound for this kernel, rtol 1e-11 and atol 1e-13 max|ref|, with the maximum taken per block (pair of observables) instead of over the whole matrix:
    P x P elements are ~ 1e16 times xi x xi elements, so that the whole-matrix maximum would let any number pass for a xi x xi block next to a P x P block.  Never
    wider than the whole-matrix bound, which it therefore implies."""
    ref = np.asarray(ref)
    tol = RTOL * np.abs(ref)
    for rows in block_slices(name):
        for cols in block_slices(name):
            tol[..., rows, cols] += ATOL * np.abs(ref[..., rows, cols]).max()
    return tol
