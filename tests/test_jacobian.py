"""CPU: the Jacobian phase of the device (desilike_amd/csrc/dl_fullshape_jac.h: d P_l(k) / d theta_p, the exact derivative rows of the analytic Fisher path) run on the host
(tests/csrc/emulate_jac.cpp), against the five-point stencil of the NumPy oracle's theory and against the gradient phase (the same sums, contracted in reverse mode)."""
import numpy as np
import pytest

from golden_utils import load_golden, spec_from_golden, observable_constants
from oracle import np_oracle as orc

H = 1e-3          # the stencil of tests/test_fisher.py:183-192
APMODES = {0: '', 1: 'qiso', 2: 'qap', 3: 'qisoqap'}


def oracle_theory(g, names, row, apmode=0):
    """The concatenated theory vector (every observable's [n_ell, n_kin] block, flattened) of the oracle at one theta row."""
    p = dict(g.get('fixed', {}), **dict(zip(names, row)))
    if apmode: p['qpar'], p['qper'] = orc.ap_qparqper(APMODES[apmode], 1. / 3., **p)
    blocks, iobs = [], 0
    while 'obs{:d}'.format(iobs) in g:
        c = observable_constants(g, iobs)
        tracer = str(c.get('tracer', ''))
        prefix = tracer + '.' if tracer else ''
        q = dict(p, b1=(p[prefix + 'b1'],) * 2, sn0=p.get(prefix + 'sn0', 0.))
        if c['template'] == 'fixed': q.pop('dm', None)
        blocks.append(orc.fullshape_observable(c, q)['power'].ravel())
        iobs += 1
    return np.concatenate(blocks)


def stencil_jacobian(theory, theta):
    """[B, P, K] by the five-point stencil of step H."""
    out = []
    for row in theta:
        rows = []
        for ip in range(len(row)):
            def f(x):
                shifted = row.copy(); shifted[ip] += x
                return theory(shifted)
            rows.append((-f(2 * H) + 8 * f(H) - 8 * f(-H) + f(-2 * H)) / (12 * H))
        out.append(rows)
    return np.array(out)


def make_case(case):
    """(golden, names, spec, theta, apmode) of a named case; the AP modes reinterpret the first two theta columns of the config-2 fixture."""
    if case in ('cfg2', 'cfg2_dn', 'cfg2_dn_only', 'cfg2_ells5', 'qiso', 'qap', 'qisoqap'):
        g = load_golden('cfg2_shapefit_window')
    elif case == 'cfg5':
        g = load_golden('cfg5_two_tracers')
    else:
        g = load_golden('cfg1_kaiser_nowindow')
    if case == 'cfg2_ells5':                                                       # five multipoles: the NL = 5 accumulators; the window reads nothing of the two new blocks
        from numpy.polynomial import legendre as npleg
        c = g['obs0']
        assert tuple(c['ellsin']) == (0, 2, 4)
        wmu = c['wmu_ell'][0]                                                      # (ell = 0: the bare Gauss-Legendre weights)
        c['wmu_ell'] = np.vstack([c['wmu_ell']] + [wmu * (2 * ell + 1) * npleg.legval(c['mu'], [0.] * ell + [1.]) for ell in (6, 8)])
        c['ellsin'] = np.array([0, 2, 4, 6, 8])
        c['matrix_full'] = np.hstack([c['matrix_full'], np.zeros((c['matrix_full'].shape[0], 2 * c['kin'].size))])
        c['shotnoisein'] = np.append(c['shotnoisein'], [0., 0.])
    names = [str(n) for n in g['names']]
    spec = spec_from_golden(g)
    theta = g['theta'][:2].copy()
    apmode = 0
    inputs = spec['observables'][0]['inputs']
    if case in ('qiso', 'qap', 'qisoqap'):
        apmode = {'qiso': 1, 'qap': 2, 'qisoqap': 3}[case]
        spec['observables'][0]['apmode'] = np.array([apmode])
        inputs['qpar'], inputs['qper'] = (-1, 1.), (-1, 1.)
        if case == 'qiso': names[0] = 'qiso'; inputs['qiso'] = (0, 1.)          # (column 1 then reaches nothing: its row must be zero)
        if case == 'qap': names[1] = 'qap'; inputs['qap'] = (1, 1.)
        if case == 'qisoqap': names[:2] = ['qiso', 'qap']; inputs['qiso'], inputs['qap'] = (0, 1.), (1, 1.)
    if case == 'cfg2_dn':                                                          # dm and dn both sampled: three spline passes
        P = len(names)
        names.append('dn')
        spec['n_params'] = np.array([P + 1])
        spec['priors'] = np.vstack([spec['priors'], [0., -0.5, 0.5, 0., 1.]])
        inputs['dn'] = (P, 0.)
        theta = np.column_stack([theta, [0.02, -0.03]])
    if case == 'cfg2_dn_only':                                                     # dm fixed at 0.01, dn sampled in its column: pass 1 is skipped, pass 2 runs
        idm = names.index('dm')
        names[idm] = 'dn'
        inputs['dm'], inputs['dn'] = (-1, 0.01), (idm, 0.)
        g['fixed'] = {'dm': 0.01}
    if case == 'fixed':                                                            # fixed template: the dm column reaches nothing
        spec['observables'][0]['template'] = np.array([0])
        inputs['dm'] = (-1, 0.)
        g['obs0']['template'] = 'fixed'
    return g, names, spec, theta, apmode


CASES = ['cfg2', 'cfg5', 'cfg2_dn', 'cfg2_dn_only', 'cfg2_ells5', 'qiso', 'qap', 'qisoqap', 'fixed']


@pytest.mark.parametrize('case', CASES)
def test_jacobian_rows_vs_oracle_stencil(case):
    from jacobian_emulation import JacobianEmulation
    g, names, spec, theta, apmode = make_case(case)
    emu = JacobianEmulation(spec)
    k_pad = (emu.n_cols + 127) // 128 * 128 + 128              # (padding columns present: they must come back as zeros)
    jac = emu.eval_jac(theta, k_pad=k_pad)
    assert jac is not None and jac.shape == (len(theta), len(names), k_pad)
    assert (jac[..., emu.n_cols:] == 0.).all()
    ref = stencil_jacobian(lambda row: oracle_theory(g, names, row, apmode=apmode), theta)
    assert ref.shape == jac[..., :emu.n_cols].shape
    # a column that reaches nothing: the analytic row is exactly zero; the oracle's stencil of a constant is zero only to its own rounding, a few roundings of 8 |theory|
    # in the four-term sum, divided by 12 H (no relative bound exists for a column whose largest entry is zero)
    unreached = {'qiso': ['qper'], 'qap': ['qpar'], 'fixed': ['dm']}.get(case, [])
    floor = 16. * np.finfo('f8').eps * np.abs(oracle_theory(g, names, theta[0], apmode=apmode)).max() / (12. * H)
    for ip, name in enumerate(names):
        scale = np.abs(ref[:, ip]).max()
        err = np.abs(jac[:, ip, :emu.n_cols] - ref[:, ip]).max()
        print('{} d / d {}: max |error| = {:.3e} of scale {:.3e}'.format(case, name, err, scale))
        if name in unreached:
            assert (jac[:, ip] == 0.).all() and scale <= floor, (case, name, scale, floor)
        else:
            assert err <= 1e-8 * scale, (case, name, err, scale)
    if case == 'cfg5':   # namespaced b1 / sn0 rows are zero in the other observable's block
        n0 = g['obs0']['kin'].size * len(g['obs0']['ellsin'])
        for ip, name in enumerate(names):
            if '.' not in name: continue
            other = slice(n0, emu.n_cols) if name.startswith(str(g['obs0']['tracer'])) else slice(0, n0)
            assert (jac[:, ip, other] == 0.).all(), name


@pytest.mark.parametrize('case', CASES)
def test_jacobian_contracted_equals_gradient_phase(case):
    """Forward and reverse mode are the same sums in another order: J . Y against dl_fs_grad_phase3 + dl_fs_grad_chain on the same random Y, 1e-12 of the largest component."""
    from jacobian_emulation import JacobianEmulation
    g, names, spec, theta, apmode = make_case(case)
    emu = JacobianEmulation(spec)
    Y = np.random.RandomState(42).standard_normal((len(theta), emu.n_cols))
    jac = emu.eval_jac(theta)
    grad = emu.eval_grad_given_y(theta, Y)
    forward = np.einsum('bpk,bk->bp', jac, Y)
    err = np.abs(forward - grad).max()
    print('{}: max |J.Y - gradient phase| = {:.3e} of {:.3e}'.format(case, err, np.abs(grad).max()))
    assert err <= 1e-12 * np.abs(grad).max()


def test_jacobian_out_of_scope():
    from jacobian_emulation import JacobianEmulation
    g = load_golden('cfg2v_eft_damping_qisoqap')   # counter terms and damping: outside dl_fs_grad_applicable
    assert JacobianEmulation(spec_from_golden(g)).eval_jac(g['theta'][:1]) is None


def test_jacobian_under_sanitizers():
    """The host build of the Jacobian phase under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only), driven through the cases of this file in a child interpreter
    with libasan preloaded; any report fails the test."""
    import os, subprocess, sys
    from jacobian_emulation import build_jacobian_emulation
    build_jacobian_emulation(sanitize=True)
    libasan = subprocess.check_output(['g++', '-print-file-name=libasan.so']).decode().strip()
    assert os.path.isabs(libasan) and os.path.isfile(libasan), 'libasan not found: the sanitizer run of the Jacobian phase is part of this suite'
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys; sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})\n'
            'import test_jacobian as t\n'
            'for case in ["cfg5", "cfg2_dn", "cfg2_dn_only", "cfg2_ells5", "qisoqap", "fixed"]: t.test_jacobian_contracted_equals_gradient_phase(case)\n'
            't.test_jacobian_out_of_scope()\n'
            'print("sanitized jacobian ok")\n').format(here=here, root=os.path.dirname(here))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', DL_EMULATION_SANITIZE='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    err = out.stderr.decode()
    assert out.returncode == 0 and 'sanitized jacobian ok' in out.stdout.decode(), err[-3000:]
    assert 'AddressSanitizer' not in err and 'runtime error' not in err, err[-3000:]
