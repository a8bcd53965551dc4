"""CPU: the prior-box fixtures (tests/golden/make_priorbox_fixture.py) -- that each belongs to its companion, follows the rules it was drawn by and stays small -- and the
NumPy oracle against the reference ON THEIR ROWS: the oracle is pinned on fixtures drawn from the samplers' start distribution (a few per cent of the prior range around
the fiducial point); here the same comparisons run at the centre, the corners, the faces and uniform points of the whole prior box, at the tolerances of the tests that
pin each family (tests/test_oracle.py, test_oracle_kaiser_xi.py, test_oracle_bao.py, test_bao_phaseshift.py, test_turnover.py, test_bands.py, test_oracle_tns.py, test_oracle_png.py, test_oracle_emulator.py).  Every GPU test that trusts the oracle away from the
fiducial point rests on this.  One term is added to the absolute tolerances on the theory vector: four roundings of the reference's own shot-noise subtraction
(priorbox_utils.shotnoise_rounding, measured in long double), which the start distribution never made visible.

The oracle works from the flat ``dl_config`` keys of the companion (tests/phaseshift_oracle.py, tests/wigglesplit_oracle.py do the same), so the window -- and for
correlation functions the folded Hankel operator -- is the companion's; the theory in front of it is the oracle's."""
import os

import numpy as np
import pytest

from oracle import np_oracle as orc
import phaseshift_oracle as pso
import priorbox_utils as pbu

NAMES = list(pbu.FIXTURES)
_loaded = {}


def load(name):
    if name not in _loaded:
        _loaded[name] = (pbu.load_priorbox(name),) + pbu.load_companion(name)
    return _loaded[name]


# ---- hygiene ----------------------------------------------------------------------------------------------------------------------------------
def test_the_28_fixtures_are_there_and_small():
    assert len(NAMES) == 28
    assert any((~np.isfinite(load(name)[2]['priors'].reshape(-1, 5)[:, 1:3])).any() and np.isfinite(load(name)[0]['ref_width']).any() for name in NAMES)      # (the open-side rule is exercised)
    sizes = [os.path.getsize(pbu.priorbox_path(name)) for name in NAMES]
    assert max(sizes) <= pbu.MAX_BYTES and sum(sizes) <= pbu.MAX_TOTAL_BYTES


@pytest.mark.parametrize('name', NAMES)
def test_fixture_belongs_to_its_companion(name):
    g, companion, cfg = load(name)
    assert str(g['cfg_sha']) == pbu.cfg_sha(companion)
    assert [str(n) for n in g['names']] == [str(n) for n in companion['names']]
    assert not any(key.startswith('cfg/') for key in g) and not any('time' in key or 'seconds' in key for key in g)
    nrows = pbu.FIXTURES[name][0]
    ndata = sum(cfg['obs{:d}.flatdata'.format(iobs)].size for iobs in range(int(cfg['n_obs'][0])))
    assert g['theta'].shape == (nrows, len(g['names'])) and g['flattheory'].shape == (nrows, ndata)
    for key in ['row_kind', 'row_bad', 'loglikelihood', 'logprior', 'logposterior']: assert g[key].shape == (nrows,), key


@pytest.mark.parametrize('name', NAMES)
def test_box_follows_the_priors(name):
    g, companion, cfg = load(name)
    names = [str(n) for n in g['names']]
    priors, box = cfg['priors'].reshape(-1, 5), g['box']
    open_side = ~np.isfinite(priors[:, 1:3]) & (priors[:, 0] == 0)[:, None]          # sides of flat priors without a limit: value -+ 5 widths of the start distribution
    assert np.array_equal(np.isfinite(g['ref_width']), open_side.any(axis=1)) and (g['ref_width'][open_side.any(axis=1)] > 0.).all()
    rule = pbu.box_from_priors(priors, value=g['value'], ref_width=np.nan_to_num(g['ref_width']))
    assert np.isfinite(rule).all()
    if open_side.any(): assert np.array_equal(rule[open_side], (g['value'][:, None] + np.array([-5., 5.]) * g['ref_width'][:, None])[open_side])
    shrunk = np.zeros(box.shape, dtype=bool)
    for pname, sides in pbu.SHRUNK.get(name, {}).items():
        for side, value in enumerate(sides):
            if value is not None:
                shrunk[names.index(pname), side] = True
                assert box[names.index(pname), side] == value and rule[names.index(pname), 0] <= value <= rule[names.index(pname), 1]
    assert np.array_equal(box[~shrunk], rule[~shrunk])
    assert np.isfinite(box).all() and (box[:, 0] < box[:, 1]).all()
    # every row inside the box, the box inside the prior limits
    assert (g['theta'] >= box[:, 0]).all() and (g['theta'] <= box[:, 1]).all()
    assert (box[:, 0] >= priors[:, 1]).all() and (box[:, 1] <= priors[:, 2]).all()


@pytest.mark.parametrize('name', NAMES)
def test_rows_are_of_their_kinds(name):
    g, companion, cfg = load(name)
    priors, box, theta, kinds = cfg['priors'].reshape(-1, 5), g['box'], g['theta'], g['row_kind']
    nrows, ncorner = pbu.FIXTURES[name]
    centre = box.mean(axis=1)
    assert kinds[0] == pbu.KIND_CENTRE and np.array_equal(theta[0], centre) and (kinds == pbu.KIND_CENTRE).sum() == 1
    cols = pbu.corner_columns(priors, ncorner)
    ncorner = min(ncorner, int(pbu.finite_uniform(priors).sum()))       # ('cfg4_flexible': three parameters have finite uniform limits, the multipliers are normal)
    assert len(cols) == ncorner >= 3
    others = np.setdiff1d(np.arange(len(box)), cols)
    corners = theta[kinds == pbu.KIND_CORNER]
    assert len(corners) == 2**ncorner >= 8
    assert ((corners[:, cols] == box[cols, 0]) | (corners[:, cols] == box[cols, 1])).all() and np.array_equal(corners[:, others], np.tile(centre[others], (len(corners), 1)))
    assert len({tuple(row) for row in corners[:, cols] == box[cols, 1]}) == 2**ncorner        # every corner occurs
    faces = theta[kinds == pbu.KIND_ALL]
    assert len(faces) == 3 and np.array_equal(faces[0], box[:, 0]) and np.array_equal(faces[1], box[:, 1]) and np.array_equal(faces[2], box[np.arange(len(box)), np.arange(len(box)) % 2])
    ones = theta[kinds == pbu.KIND_ONE]
    assert len(ones) <= 24 and (((ones != centre).sum(axis=1)) == 1).all()
    assert np.array_equal(pbu.rows_in_box(box, priors, nrows, ncorner, 0)[1], kinds)
    uniform = theta[kinds == pbu.KIND_UNIFORM]
    assert ((uniform > box[:, 0]) & (uniform < box[:, 1])).all()
    if name in pbu.PLAIN: assert nrows == 64
    else: assert nrows == 16


@pytest.mark.parametrize('name', NAMES)
def test_reference_values(name):
    g, companion, cfg = load(name)
    bad = g['row_bad']
    assert bad.mean() <= pbu.MAX_BAD
    assert np.isfinite(g['logprior'][~bad]).all() and np.isfinite(g['loglikelihood'][~bad]).all() and np.isfinite(g['flattheory'][~bad]).all()
    assert np.isnan(g['loglikelihood'][bad]).all()
    if name in pbu.PLAIN:
        assert np.allclose(g['loglikelihood'][~bad] + g['logprior'][~bad], g['logposterior'][~bad], rtol=1e-15, atol=0.)
        priors = [dict(dist=['uniform', 'norm'][int(row[0])], limits=(row[1], row[2]), loc=row[3], scale=row[4]) for row in cfg['priors'].reshape(-1, 5)]
        assert np.allclose(orc.logprior(g['theta'][~bad], priors), g['logprior'][~bad], rtol=1e-13, atol=1e-13)
    else:
        for i in np.flatnonzero(~bad):
            assert g['logposterior'][i] == pbu.marginalised_logposterior(g['marg_c'][i], g['marg_g'][i], g['marg_H'][i], cfg['marg.kind'])[0]
            assert abs(g['marg_c'][i] - (g['loglikelihood'][i] + g['logprior'][i])) <= 1e-13 * abs(g['marg_c'][i])      # the quadratic's value at x0 is the unsolved pipeline's


# ---- the oracle over the box ------------------------------------------------------------------------------------------------------------------
def kaiser_flattheory(cfg, row):
    """(EFT-like) Kaiser multipoles on the ShapeFit, turn-over or band template from the flat keys: power_template.py:749, full_shape.py:336-364, 545-550, 628-634; the window (for
    correlation functions: with the Hankel operator folded in) and the shot-noise terms as dl_host.hpp::dl_build_window folds them."""
    flat = []
    for iobs in range(int(cfg['n_obs'][0])):
        c = pso.observable_keys(cfg, iobs)
        template = int(c['template'][0])
        qpar, qper = pso._ap(c, row)
        nell, nkin = len(c['ells_in']), len(c['kin'])
        ells = tuple(int(ell) for ell in c['ells_in'])
        f = float(c['f_fid'][0]) * pso._input(c, 'df', row, 1.)
        if template == 1:      # ShapeFit
            pk11 = c['pk_dd_fid'] * orc.shapefit_factor(c['k_t'], float(c['kp'][0]), float(c['a'][0]), dm=pso._input(c, 'dm', row, 0.), dn=pso._input(c, 'dn', row, 0.))
        elif template == 2:    # turn-over, power_template.py:1326-1333
            pk11 = orc.turnover_pk(c['k_t'], float(c['kto_fid'][0]), float(c['pkto_fid'][0]), m=pso._input(c, 'm', row, 0.6), n=pso._input(c, 'n', row, 0.9),
                                   qto=pso._input(c, 'qto', row, 1.), dpto=pso._input(c, 'dpto', row, 1.))
        else:                  # velocity bands, power_template.py:955-961 (``pk_dd_fid`` holds P_tt_fid / f_fid^2)
            assert template == 3
            dptt = np.array([row[int(round(col))] if col >= 0 else value for col, value in c['in.band'].reshape(-1, 2)])
            pk11 = c['pk_dd_fid'] * (1. + (dptt - 1.).dot(c['band_templates'].reshape(len(dptt), -1))) / pso._input(c, 'df', row, 1.)**2
        dd, dt, tt = orc.kaiser_pktable(c['kin'], c['mu'], c['wmu_ell'].reshape(nell, -1), c['k_t'], pk11, f, qpar=qpar, qper=qper,
                                        sigmapar=pso._input(c, 'sigmapar', row, 0.), sigmaper=pso._input(c, 'sigmaper', row, 0.))
        nd = float(c['nd'][0])
        power = orc.kaiser_tracer_power(ells, dd, dt, tt, nd, pso._input(c, 'b1X', row, 1.), pso._input(c, 'b1Y', row, 1.), pso._input(c, 'sn0', row, 0.))
        if 'ct_matrix' in c:
            value = lambda pair: row[int(round(pair[0]))] if pair[0] >= 0 else pair[1]   # noqa: E731
            ct = [value(pairs[0]) + value(pairs[1]) for pairs in c['in.ct'].reshape(-1, 2, 2)]
            sn = [value(pair) for pair in c['in.sn'].reshape(-1, 2)]
            power = orc.eftlike_addon(power, ells, dd, c['ct_matrix'].reshape(nell, nkin, -1), ct, c['sn_matrix'].reshape(nell, nkin, -1), sn, nd)
        W, bias = pso.window(c)
        flat.append(W.dot(np.ravel(power)) + bias)
    return np.concatenate(flat)


_tns_kernels = {}


def tns_flattheory(cfg, row):
    """One-loop TNS multipoles (full_shape.py:688-971) from the flat keys, as bench_configs.tns_oracle_point forms them from a fixture of its own layout."""
    c = pso.observable_keys(cfg, 0)
    assert int(cfg['n_obs'][0]) == 1 and int(c['template'][0]) == 1
    q, k11 = c['k_t'], c['tns_k11']
    key = (q.tobytes(), k11.tobytes())
    if key not in _tns_kernels: _tns_kernels[key] = orc.tns_kernels(k11, q, orc.weights_trapz(q))      # (depend on the grids only)
    nell, nkin = len(c['ells_in']), len(c['kin'])
    ells = [int(ell) for ell in c['ells_in']]
    pk_q = c['pk_dd_fid'] * orc.shapefit_factor(q, float(c['kp'][0]), float(c['a'][0]), dm=pso._input(c, 'dm', row, 0.), dn=pso._input(c, 'dn', row, 0.))
    qpar, qper = pso._ap(c, row)
    pt = orc.tns_pktable(c['kin'], c['mu'], c['wmu_ell'].reshape(nell, -1), q, pk_q, float(c['f_fid'][0]) * pso._input(c, 'df', row, 1.), qpar=qpar, qper=qper,
                         sigmav=pso._input(c, 'sigmav', row, 0.), fog='gaussian' if int(c['tns_fog'][0]) else 'lorentzian', kernels=_tns_kernels[key], k11=k11)
    nd = float(c['nd'][0])
    power = orc.tns_tracer_power(pt, nd, b1=pso._input(c, 'b1X', row, 1.), b2=pso._input(c, 'b2', row, 0.), bs=pso._input(c, 'bs', row, 0.), b3=pso._input(c, 'b3', row, 0.),
                                 sn0=pso._input(c, 'sn0', row, 0.))
    if 'ct_matrix' in c:
        value = lambda pair: row[int(round(pair[0]))] if pair[0] >= 0 else pair[1]   # noqa: E731
        ct = np.array([value(pairs[0]) + value(pairs[1]) for pairs in c['in.ct'].reshape(-1, 2, 2)])
        sn = np.array([value(pair) for pair in c['in.sn'].reshape(-1, 2)])
        power = orc.eftlike_addon(power, ells, pt['pk11'], c['ct_matrix'].reshape(nell, nkin, -1), ct, c['sn_matrix'].reshape(nell, nkin, -1), sn, nd)
    W, bias = pso.window(c)
    return W.dot(np.ravel(power)) + bias


def png_flattheory(cfg, row):
    """Scale-dependent bias from primordial non-Gaussianity (primordial_non_gaussianity.py:75-112; tracer-velocity variant 284-320) from the flat keys, as
    tests/test_oracle_png.py::png_oracle_point forms it: ``png_alpha`` is alpha(k) of the fiducial template (its first wavenumber already dropped, as ``k_t`` and
    ``pk_dd_fid`` are), alpha = sqrt(P_phi / P_dd) follows the template factor."""
    c = pso.observable_keys(cfg, 0)
    assert int(cfg['n_obs'][0]) == 1 and int(c['template'][0]) == 1
    nell = len(c['ells_in'])
    factor = orc.shapefit_factor(c['k_t'], float(c['kp'][0]), float(c['a'][0]), dm=pso._input(c, 'dm', row, 0.), dn=pso._input(c, 'dn', row, 0.))
    pk_dd, alpha = c['pk_dd_fid'] * factor, c['png_alpha'] / factor**0.5
    qpar, qper = pso._ap(c, row)
    f = float(c['f_fid'][0]) * pso._input(c, 'df', row, 1.)
    mode = 'b-p' if int(c['png_mode'][0]) else 'bphi'
    fnl, b1X, b1Y = pso._input(c, 'fnl_loc', row, 0.), pso._input(c, 'b1X', row, 1.), pso._input(c, 'b1Y', row, 1.)
    bfX = orc.png_bfnl(mode, b1X, fnl_loc=fnl, p=pso._input(c, 'pX', row, 1.), bphi=pso._input(c, 'bphiX', row, 1.))
    bfY = orc.png_bfnl(mode, b1Y, fnl_loc=fnl, p=pso._input(c, 'pY', row, 1.), bphi=pso._input(c, 'bphiY', row, 1.))
    grid = (c['kin'], c['mu'], c['wmu_ell'].reshape(nell, -1), c['k_t'], pk_dd, alpha, f)
    if 'png_velocity' in c and int(c['png_velocity'][0]):
        power = orc.png_velocity_power(*grid, 100. / float(c['png_velfac'][0]) - 1., b1X, bfX, bv=pso._input(c, 'bv', row, 1.), sigmas=pso._input(c, 'sigmas', row, 0.),
                                       sigmau=pso._input(c, 'sigmau', row, 0.), qpar=qpar, qper=qper)
    else:
        power = orc.png_tracer_power(*grid, float(c['nd'][0]), b1X, b1Y, bfX, bfY, sn0=pso._input(c, 'sn0', row, 0.), sigmasX=pso._input(c, 'sigmas', row, 0.),
                                     sigmasY=pso._input(c, 'sigmasY', row, 0.), qpar=qpar, qper=qper)
    W, bias = pso.window(c)
    return W.dot(np.ravel(power)) + bias


_ACTIVATION = {0: 'silu', 1: 'relu', 2: 'tanh'}      # emulators/conversion.py:27-34, the codes of include/desilike_amd.h


def _dense_layers(weights, widths):
    """[(kernel [in, out], bias [out]) ...] of one network from its flat weights: layer by layer, kernel row-major then bias."""
    layers, pos = [], 0
    for nin, nout in zip(widths[:-1], widths[1:]):
        layers.append((weights[pos:pos + nin * nout].reshape(nin, nout), weights[pos + nin * nout:pos + nin * nout + nout]))
        pos += nin * nout + nout
    return layers, pos


def _hidden(x, xlimits, layers, activation):
    """The last hidden layer of a network: the forward pass of orc.mlp_predict with an activation after every layer given (its output layer is folded into the window)."""
    identity = (np.eye(layers[-1][0].shape[1]), np.zeros(layers[-1][0].shape[1]))
    return orc.mlp_predict(x, xlimits, list(layers) + [identity], activation)


def _scalar_engine(c, e, x):
    """sigma8 / fsigma8: a constant, a Taylor engine or an MLP with its own output layer and y-scaler."""
    p = 'emu{:d}.'.format(e)
    if p + 'const' in c: return float(c[p + 'const'][0])
    if int(c[p + 'type'][0]) == 1:
        return float(orc.taylor_predict(x, c[p + 'center'], c[p + 'powers'].reshape(-1, len(x)), c[p + 'coef']))
    layers, _ = _dense_layers(c[p + 'weights'], [int(w) for w in c[p + 'widths']])
    return float(np.ravel(orc.mlp_predict(x, c[p + 'xlimits'].reshape(-1, 2), layers, _ACTIVATION[int(c[p + 'act'][0])], c[p + 'ylimits'].reshape(1, 2)))[0])


def emulated_flattheory(cfg, row):
    """Velocileptors tracers on an emulated perturbation-theory node from the flat keys (full_shape.py:1182-1186, 1300-1313, 1479-1488, 1577-1599; engines:
    emulators/__init__.py:471-507, emulators/conversion.py:20-98), as tests/test_oracle_emulator.py chains the oracle: engine forward passes, the 11 'pars', the 19 bias
    monomials.  Everything linear behind the engines' trunks (output layers or derivative tables, assembly, k-interpolation, window) is the companion's ``wmatrix``:
    theory vector = wmatrix . [basis_h(x) monomial_m(pars)] + offset - shotnoise_out."""
    c = pso.observable_keys(cfg, 0)
    assert int(cfg['n_obs'][0]) == 1 and 'kmask' not in c
    x = np.array([row[int(round(col))] if col >= 0 else value for col, value in c['in.x'].reshape(-1, 2)])
    vp = [row[int(round(col))] if col >= 0 else value for col, value in c['in.vp'].reshape(11, 2)]
    mode = int(c['mono_mode'][0])                 # 1 LPT physical, 2 REPT physical, 3 LPT direct, 4 REPT direct
    physical, model = mode in (1, 2), 'rept' if mode in (2, 4) else 'lpt'
    snd, fsat, sigv, nd = (float(v) for v in c['vconst'])
    sigma8, fsigma8 = _scalar_engine(c, 1, x), _scalar_engine(c, 2, x)
    names = ['b1', 'b2', 'bs', 'b3', 'alpha0', 'alpha2', 'alpha4', 'alpha6', 'sn0', 'sn2', 'sn4']
    params = {name + ('p' if physical else ''): value for name, value in zip(names, vp)}
    pars = orc.velocileptors_pars(params, sigma8, fsigma8 / sigma8, basis='physical' if physical else 'direct', model=model, snd=snd, fsat=fsat, sigv=sigv)
    monomials = orc.tablevel_combine_bias_terms_poles(np.eye(19), pars, nd=nd)
    kind = int(c['emu0.type'][0])
    if kind == 1:
        basis = np.prod((x - c['emu0.center'])**c['emu0.powers'].reshape(-1, len(x)), axis=-1)           # the monomials of orc.taylor_predict
        phi = np.outer(basis, monomials).ravel()
    elif kind == 0:
        layers, _ = _dense_layers(c['emu0.weights'], [int(w) for w in c['emu0.widths']])
        basis = np.concatenate([_hidden(x, c['emu0.xlimits'].reshape(-1, 2), layers, _ACTIVATION[int(c['emu0.act'][0])]), [1.]])
        phi = np.outer(basis, monomials).ravel()
    else:                                          # stacked layout: groups of networks, each group with its amplitude and its monomials
        widths, xlimits, activation = [int(w) for w in c['emu0.widths']], c['emu0.xlimits'].reshape(-1, 2), _ACTIVATION[int(c['emu0.act'][0])]
        per_network = sum(nin * nout + nout for nin, nout in zip(widths[:-1], widths[1:]))
        phi = []
        for (t0, t1, m0, m1), scale in zip(c['emu0.groups'].reshape(-1, 4), c['emu0.scale'].reshape(-1, len(x) + 1)):
            hidden = [_hidden(x, xlimits, _dense_layers(c['emu0.weights'][t * per_network:(t + 1) * per_network], widths)[0], activation) for t in range(t0, t1)]
            phi.append(np.exp(scale[:-1].dot(x) + scale[-1]) * np.outer(np.concatenate(hidden + [[1.]]), monomials[m0:m1]).ravel())
        phi = np.concatenate(phi)
    flat = c['wmatrix'].reshape(-1, phi.size).dot(phi)
    if 'offset' in c: flat = flat + c['offset']
    return flat - c['shotnoise_out']


# family -> (fixtures, oracle theory vector from the keys, (rtol, atol in units of the row's largest magnitude, atol) on the theory vector: those of the test that pins it)
ORACLES = {'kaiser': (['cfg2_dense', 'two_tracers', 'eft_qisoqap'], kaiser_flattheory, (1e-12, 0., 1e-9)),                       # tests/test_oracle.py
           'kaiser_xi': (['kaiser_xi', 'xi_binned'], kaiser_flattheory, (1e-10, 1e-12, 0.)),                                         # tests/test_oracle_kaiser_xi.py
           'turnover': (['turnover'], kaiser_flattheory, (1e-11, 0., 1e-8)),                                                        # tests/test_turnover.py (its bound on the multipoles)
           'bands': (['bands'], kaiser_flattheory, (1e-11, 0., 1e-8)),                                                              # tests/test_bands.py
           'tns': (['tns', 'tns_eft'], tns_flattheory, (1e-11, 1e-11, 0.)),                                                         # tests/test_oracle_tns.py
           'png': (['png', 'png_velocity'], png_flattheory, (1e-11, 1e-12, 0.)),                                                   # tests/test_oracle_png.py
           'emulated': (['cfg3', 'cfg3_taylor', 'cfg3_taylor_standard', 'cfg3_stacked', 'cfg3_stacked_lpt'], emulated_flattheory, (1e-12, 0., 1e-9)),   # tests/test_oracle_emulator.py
           'bao': (['cfg4_pk', 'cfg4_xi', 'cfg4_resummed', 'cfg4_resummed_xi_binned', 'cfg4_flexible', 'cfg4_models', 'cfg4_pk_pcs', 'cfg4_xi_pcs2'],
                   lambda cfg, row: pso.flattheory(cfg, row)[0], (1e-11, 1e-13, 0.)),                                               # tests/test_oracle_bao.py
           'phaseshift': (['phaseshift_pk', 'phaseshift_xi'], lambda cfg, row: pso.flattheory(cfg, row)[0], (1e-11, 1e-13, 0.))}    # tests/test_bao_phaseshift.py
ORACLE_CASES = [(family, name) for family, (names, _, _) in ORACLES.items() for name in names]


@pytest.mark.parametrize('family,name', ORACLE_CASES)
def test_oracle_over_the_prior_box(family, name):
    g, companion, cfg = load(name)
    flattheory, (rtol, atol_rel, atol) = ORACLES[family][1:]
    flatdata, precision = pso.flatdata(cfg), pso.precision(cfg)
    worst = {}
    for i in np.flatnonzero(~g['row_bad']):
        flat = flattheory(cfg, g['theta'][i])
        ref, ref_ll = g['flattheory'][i], g['loglikelihood'][i]
        logl = orc.gaussian_loglikelihood(flat, flatdata, precision)[0]
        kind = int(g['row_kind'][i])
        scale = np.abs(ref).max()
        worst[kind] = np.maximum(worst.get(kind, 0.), [abs(logl - ref_ll) / max(1., abs(ref_ll)), np.abs(flat - ref).max() / scale if scale > 0. else np.abs(flat - ref).max()])
        assert np.allclose(flat, ref, rtol=rtol, atol=atol + atol_rel * scale + pbu.shotnoise_rounding(cfg)), (name, i, np.abs(flat - ref).max(), scale)
        assert abs(logl - ref_ll) <= 1e-10 * max(1., abs(ref_ll)), (name, i, logl, ref_ll)
    print(name, 'oracle against reference by row kind (logL error / max(1, |logL|), theory error / row maximum):', {kind: tuple(float('{:.1e}'.format(v)) for v in value) for kind, value in sorted(worst.items())})
