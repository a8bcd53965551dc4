"""CPU: the extended-precision reference of the analytic marginalisation (tests/marg_reference.py) against the float64 oracle ``oracle.np_oracle.solve_marginalized`` on the
cases of tests/test_oracle_marg.py, and the INPUT CONDITIONS of every case of the GPU sweep tests/test_gpu_marg_counts.py, computed with the oracle's theory chain (no device):
 (a) chi2(x0) <= 1e4 on every compared row: the marginalised value is assembled from -G00 / 2 with G00 = chi2(x0), whose rounding is eps chi2(x0) in absolute terms;
 (b) the float64 oracle agrees with the extended-precision reference to 1e-11 max(1, |.|) on every compared row, every quantity and every '.marg' pattern.
With both, the tolerances of the sweep (1e-10 on the values, 1e-8 on the solution) test the kernels, not the conditioning of the cases."""
import numpy as np
import pytest

from oracle import np_oracle as orc
from golden_utils import load_golden, observable_constants
import marg_reference as mr
import marg_counts_cases as mc

KEYS = ['loglikelihood', 'logprior_solved', 'x', 'likelihood_hessian']


def worst(sol, ref):
    """max over the compared quantities of |float64 oracle - reference| / max(1, |reference|)."""
    return max(float((np.abs(np.asarray(sol[key]) - np.asarray(ref[key])) / np.maximum(1., np.abs(ref[key]))).max()) for key in KEYS)


@pytest.mark.parametrize('ip', range(6))
def test_reference_vs_oracle_on_reference_grid_fixture(ip):
    """The rows of fixture marg_sn0_grid (tests/test_oracle_marg.py::test_marginalisation_vs_reference_grid), Delta taken at x0 = 0 and at x0 = 0.3, '.marg' and '.best'.

    Measured |float64 oracle - reference| / max(1, |reference|): at most 2.9e-15 (row 3, x0 = 0, '.best').  The fixture's data sit at chi2(x0 = 0) = 1.8e4 (1.2e3 at x0 = 0.3): with
    the 120 x 120 terms of chi2(x0), T P Delta and T P T^T accumulated in float64 the oracle was at 1.0027e-12 on row 0 (up to 2.6e-13 on the others) -- its own rounding entering in
    absolute terms, which is why ``solve_marginalized`` now accumulates these sums, and the three cancelling terms of the value, in long double."""
    g = load_golden('marg_sn0_grid')
    assert len(g['theta']) == 6
    c = observable_constants(g)
    loc, scale = g['sn0_prior']
    precision = mr.exact_ints(g['precision'])
    T = (g['flattheory_sn0_1'][ip] - g['flattheory_sn0_0'][ip])[None, :]
    flatdiff = g['flattheory_sn0_0'][ip] - c['flatdata']
    errors = {}
    for x0, diff in [(0., flatdiff), (0.3, flatdiff + 0.3 * T[0])]:
        G = mr.marg_gram(diff, T, precision)
        for marg in [True, False]:
            sol = orc.solve_marginalized(diff, T, g['precision'], x0=[x0], prior_loc=[loc], prior_scale=[scale], marg_mask=[marg])
            ref = mr.marg_from_gram(G, [x0], [loc], [scale], [marg])
            errors[x0, marg] = worst(sol, ref)
    print('row {:d}: {}'.format(ip, {key: '{:.2e}'.format(value) for key, value in errors.items()}))
    assert max(errors.values()) <= 1e-12, errors


def test_reference_vs_oracle_closed_form_case():
    # the flat-prior, diagonal-precision case of tests/test_oracle_marg.py, and the same rows with Gaussian priors, a '.best' parameter and a dense precision
    rng = np.random.RandomState(0)
    n = 30
    T = rng.standard_normal((2, n))
    d = rng.standard_normal(n) * 3.
    prec = rng.uniform(0.5, 2., n)
    A = rng.standard_normal((n, n))
    for precision in [prec, A.dot(A.T) + n * np.eye(n)]:
        for scale, mask in [([np.inf, np.inf], [True, True]), ([2., np.inf], [True, False]), ([0.5, 3.], [False, False])]:
            args = dict(x0=[0.1, -0.2], prior_loc=[0.3, 0.], prior_scale=scale, marg_mask=mask)
            sol, ref = orc.solve_marginalized(d, T, precision, **args), mr.marg_reference(d, T, precision, **args)
            assert worst(sol, ref) <= 1e-12, (scale, mask, worst(sol, ref))
            slow = mr.marg_reference(d, T, precision, exact=False, **args)      # the Gram matrix term by term in mpmath: the same float64 numbers
            assert all(np.array_equal(ref[key], slow[key]) for key in KEYS)


def test_exact_ints_are_exact():
    a = np.array([0., 1., -3.5, 1e-300, 2.**-1074, 1.7976931348623157e308, np.pi, -1e-17])
    ints, e = mr.exact_ints(a[:5])
    from fractions import Fraction
    assert all(Fraction(int(i)) * Fraction(2)**e == Fraction(float(v)) for i, v in zip(ints, a[:5]))
    ints, e = mr.exact_ints(a[5:])
    assert all(Fraction(int(i)) * Fraction(2)**e == Fraction(float(v)) for i, v in zip(ints, a[5:]))


def check_conditions(case, label):
    precision = mr.exact_ints(case.precision)
    chi2_max, err_max = 0., 0.
    for i in range(mc.NROWS):
        G = mr.marg_gram(case.delta[i], case.T[i], precision)
        for name, mask in mc.mask_patterns(case.n_s, seed=case.n_s):
            ref = mr.marg_from_gram(G, case.x0, case.prior_loc, case.prior_scale, mask)
            sol = orc.solve_marginalized(case.delta[i], case.T[i], case.precision, case.x0, case.prior_loc, case.prior_scale, mask)
            chi2_max, err_max = max(chi2_max, ref['chi2_x0']), max(err_max, worst(sol, ref))
    print('{}: n = {:d}, n_s = {:d}: (a) max chi2(x0) = {:.1f} <= 1e4, (b) float64 oracle vs reference {:.1e} <= 1e-11'.format(label, case.n, case.n_s, chi2_max, err_max))
    assert chi2_max <= 1e4, (label, chi2_max)
    assert err_max <= 1e-11, (label, err_max)
    assert all(loc != x0 for loc, x0, scale in zip(case.prior_loc, case.x0, case.prior_scale) if np.isfinite(scale))   # Gaussian priors off the expansion point


@pytest.mark.parametrize('n,n_s', mc.CASES, ids=mc.CASE_IDS)
def test_sweep_conditions_residual_route(n, n_s):
    check_conditions(mc.get_case(n, n_s), 'residual ' + mc.expected_branch(n, n_s))


@pytest.mark.parametrize('kind,basis,count', mc.GRAM_CASES, ids=mc.GRAM_CASE_IDS)
def test_sweep_conditions_gram_route(kind, basis, count):
    check_conditions(mc.get_gram_case(kind, basis, count), 'gram {} {}'.format(kind, basis))


def test_sweep_reaches_every_count_and_branch():
    """Every n_s = 1 .. 16 and each of the four kernels / branches of the residual route has a case; the priors of the sweep mix Gaussian and flat."""
    assert {n_s for n, n_s in mc.CASES} == set(range(1, 17))
    branches = {mc.expected_branch(n, n_s) for n, n_s in mc.CASES}
    assert branches == {'staged<true,true>', 'staged<true,true>+attribute', 'unstaged<true,false>', 'serial<false,false>'}
    # the shapes named for the thresholds sit on the side they are meant to
    assert mc.staged_lds_bytes(20, 3) == 4 * 512 * 8                                                        # the 512-double floor
    assert mc.staged_lds_bytes(120, 11) <= 48 * 1024 < mc.staged_lds_bytes(120, 12)
    assert mc.staged_lds_bytes(360, 7) <= 96 * 1024 < mc.staged_lds_bytes(360, 8)
    assert mc.staged_lds_bytes(504, 5) <= 96 * 1024 < mc.staged_lds_bytes(512, 5)
    assert {count for kind, basis, count in mc.GRAM_CASES if kind == 'mlp'} == set(range(1, 8))
