"""WiggleSplitPowerSpectrumTemplate (reference power_template.py:1150-1214) without a GPU: the NumPy oracle against fixtures captured from the reference
(tests/golden/make_wigglesplit_fixture.py), the mirror class against the reference's parameter file and keys, and the phases of the template kernel
(csrc/dl_wigglesplit.h) run on the CPU (tests/csrc/emulate_wigglesplit.cpp): as a shared object against the fixtures, and as a program of its own under the sanitizers.
Bounds: the project's standing ones (tests/test_bao_phaseshift.py): template and theory rtol 1e-11 + 1e-12 max, logL 1e-10 max(1, |logL|)."""
import os
import subprocess

import numpy as np
import pytest

import wigglesplit_oracle as wso
import wigglesplit_utils as wsu


@pytest.mark.parametrize('name', wsu.FIXTURES)
def test_oracle_vs_reference(name):
    g, cfg = wsu.load_fixture(name)
    assert g['theta'].shape[0] == 48
    for i in range(48):
        row = g['theta'][i]
        flat, powers, templates = wso.flattheory(cfg, row)
        assert wsu.close(templates[0], g['pk_dd'][i]) <= 1.
        for iobs, power in enumerate(powers):
            assert wsu.close(np.ravel(power), g['theory_obs{:d}'.format(iobs)][i]) <= 1., (i, iobs)
        assert np.allclose(flat, g['flattheory'][i], rtol=1e-11, atol=1e-12 * np.abs(g['flattheory'][i]).max())
        logl = wso.loglikelihood(cfg, row)
        assert abs(logl - g['loglikelihood'][i]) <= 1e-10 * max(1., abs(g['loglikelihood'][i]))
        df = row[[str(n) for n in g['names']].index('df')]
        assert g['f'][i] == float(cfg['obs0.f_fid'][0]) * df


@pytest.mark.parametrize('name', wsu.FIXTURES)
def test_corner_rows_are_on_the_corners(name):
    g, cfg = wsu.load_fixture(name)
    names = [str(n) for n in g['names']]
    corners = [('qbao', 0.8), ('qbao', 1.2), ('dm', -3.), ('dm', 3.), ('df', 0.5), ('df', 1.5)]
    for row, (pname, value) in enumerate(corners):
        assert g['theta'][row, names.index(pname)] == value
        lo, hi = g['prior_limits'][names.index(pname)]
        assert value in (lo, hi) or pname == 'df'
    assert np.isfinite(g['logprior']).all()          # every row is inside the priors, the corners included
    for pname, (lo, hi) in [('qbao', (0.8, 1.2)), ('qap', (0.8, 1.2)), ('dm', (-3., 3.)), ('df', (0.5, 1.5))]:
        column = g['theta'][:, names.index(pname)]
        assert lo <= column.min() and column.max() <= hi and column.max() - column.min() > 0.8 * (hi - lo)
    # the inner grid: 2000-point geomspace without its outer octaves, uniform in log10 k; (1e-5, 1e2) leaves 1828 knots, (1e-4, 30) leaves 1780
    k = cfg['obs0.ws_k']
    assert len(k) == (1780 if name == 'tophat_eft' else 1828)
    assert np.abs(np.diff(np.log10(k)) / np.diff(np.log10(k)).mean() - 1.).max() < 1e-11


def test_mirror_parameters_match_reference():
    from desilike_amd.theories.galaxy_clustering import WiggleSplitPowerSpectrumTemplate, BasePowerSpectrumTemplate
    assert issubclass(WiggleSplitPowerSpectrumTemplate, BasePowerSpectrumTemplate)
    for name in ['kaiser', 'tophat_eft']:
        g, like = wsu.make_likelihood(name)
        assert like.varied_params.names() == [str(n) for n in g['names']]
        limits = np.array([like.varied_params[n].prior.limits for n in like.varied_params.names()], dtype='f8')
        assert np.array_equal(limits, g['prior_limits'])
        template = like.observables[0].wmatrix.theory.template
        mine = [param for param in template.params]
        assert [param.basename for param in mine] == [str(n) for n in g['params/names']] == ['qbao', 'qap', 'df', 'dm']
        for i, param in enumerate(mine):
            assert param.value == g['params/value'][i] and not param.fixed and not g['params/fixed'][i]
            assert tuple(param.prior.limits) == tuple(g['params/prior_limits'][i]) and tuple(param.ref.limits) == tuple(g['params/ref_limits'][i])
            assert param.delta[0] == param.value and param.delta[1] == param.delta[2] == g['params/delta'][i]      # (centre, step below, step above)
            assert param.latex() == str(g['params/latex'][i])
        assert template.params['dm'].delta[1:] == (0.005, 0.005) and template.apmode == 'qap'
        # the constants the kernel receives are the reference's own, to the last bit
        cfg = wsu.load_fixture(name)[1]
        spec = like._spec({}, like._flatdata_list(), like.precision)['observables'][0]
        for key in ['k_t', 'ws_k', 'ws_pknow', 'ws_kfid', 'ws_pk_tt_fid', 'ws_pknow_tt_fid', 'ws_r', 'ws_kernel', 'ws_kp', 'ws_fsigmar_fid', 'f_fid', 'template', 'theory', 'apmode']:
            assert np.array_equal(np.ravel(spec[key]), np.ravel(cfg['obs0.' + key])), key
        for key in ['qbao', 'dm', 'df', 'qap']:
            assert tuple(spec['inputs'][key]) == tuple(cfg['obs0.in.' + key]), key


def test_mirror_routing_and_refusals():
    from desilike_amd.fiducial import TabulatedFiducial, SyntheticFiducial
    from desilike_amd.theories.galaxy_clustering import (WiggleSplitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles, SimpleTracerPowerSpectrumMultipoles,
                                                         KaiserTracerCorrelationFunctionMultipoles, EFTLikeKaiserTracerPowerSpectrumMultipoles,
                                                         DampedBAOWigglesTracerPowerSpectrumMultipoles, TNSTracerPowerSpectrumMultipoles, PNGTracerPowerSpectrumMultipoles,
                                                         EmulatedTracerPowerSpectrumMultipoles)
    # the Kaiser family takes the template; a synthetic fiducial is tabulated on the 2000-point grid first
    for cls in [KaiserTracerPowerSpectrumMultipoles, SimpleTracerPowerSpectrumMultipoles, EFTLikeKaiserTracerPowerSpectrumMultipoles, KaiserTracerCorrelationFunctionMultipoles]:
        theory = cls(template=WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic'))
        spec = theory._theory_spec()
        assert int(spec['template'][0]) == 5 and int(spec['apmode'][0]) == 2 and theory._input_map()['qbao'] == 'qbao'
        assert len(spec['ws_k']) == 1828 and len(spec['ws_kfid']) == 2000 and float(spec['ws_kp'][0]) == 0.05 and int(spec['ws_kernel'][0]) == 0 and float(spec['ws_r'][0]) == 8.
        assert theory.template.with_now == 'peakaverage' and theory.template.klim_wiggles == (1e-5, 1e2)
    # ... the others say so
    for cls in [DampedBAOWigglesTracerPowerSpectrumMultipoles, TNSTracerPowerSpectrumMultipoles, PNGTracerPowerSpectrumMultipoles]:
        with pytest.raises(NotImplementedError, match='Kaiser'):
            cls(template=WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic')).initialize()
    with pytest.raises(NotImplementedError, match='Kaiser'):
        EmulatedTracerPowerSpectrumMultipoles(template=WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic')).initialize()
    template = WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic', only_now=True)
    for attempt in range(2):      # (the second call raises again: the template is not left half initialised)
        with pytest.raises(NotImplementedError, match='only_now'):
            KaiserTracerPowerSpectrumMultipoles(template=template).initialize()
    with pytest.raises(ValueError, match='kernel'):
        KaiserTracerPowerSpectrumMultipoles(template=WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic', kernel='box')).initialize()
    with pytest.raises(ValueError, match='TabulatedFiducial'):
        KaiserTracerPowerSpectrumMultipoles(template=WiggleSplitPowerSpectrumTemplate(z=0.5, fiducial='synthetic', pk_tt_fid=np.ones(4))).initialize()
    # a tabulated fiducial: the inner grid follows the ends of its table; theta-theta is f_fid^2 P_dd unless given
    fid = SyntheticFiducial()
    k = np.geomspace(1e-4, 30., 700)
    template = WiggleSplitPowerSpectrumTemplate(z=0.5, kernel='tophat', fiducial=TabulatedFiducial(k=k, pk_dd=fid.pk_dd(k), pknow_dd=fid.pknow_dd(k), f=0.8))
    KaiserTracerPowerSpectrumMultipoles(template=template).initialize()
    assert template.klim_wiggles == (k[0], k[-1]) and template.k_wiggles.size == 1780 and np.allclose(template.pk_tt_fid, 0.8**2 * fid.pk_dd(k), rtol=1e-13, atol=0.)   # (the provider keeps ln P: not to the bit)


@pytest.mark.parametrize('name', wsu.FIXTURES)
def test_phase_emulation_vs_reference(name):
    """The device phase functions on the CPU, all 48 points, with the kernel's 256 threads: template rows and theory rows of every observable at the standing bounds; 64
    emulated threads (another order of the quadrature sum) stay inside them too."""
    g, cfg = wsu.load_fixture(name)
    for iobs in range(int(cfg['n_obs'][0])):
        templ, power = wsu.emulate(cfg, g['theta'], iobs=iobs, nthr=256)
        assert wsu.close(templ, g['pk_dd']) <= 1.
        assert wsu.close(power, g['theory_obs{:d}'.format(iobs)]) <= 1., iobs
    templ64, _ = wsu.emulate(cfg, g['theta'][:8], nthr=64)
    assert wsu.close(templ64, g['pk_dd'][:8]) <= 1.


def test_phase_emulation_nan_and_far_rows():
    """NaN qbao / dm give NaN templates; qbao far outside the prior gives whatever the clamped table gives, without touching the neighbours."""
    g, cfg = wsu.load_fixture('kaiser')
    names = [str(n) for n in g['names']]
    theta = g['theta'][:6].copy()
    theta[1, names.index('qbao')] = np.nan
    theta[2, names.index('dm')] = np.nan
    theta[3, names.index('qbao')] = 0.3
    theta[4, names.index('qbao')] = 5.
    templ, power = wsu.emulate(cfg, theta)
    assert np.isnan(templ[1]).all() and np.isnan(templ[2]).all() and np.isnan(power[1]).all() and np.isnan(power[2]).all()
    clean = wsu.emulate(cfg, g['theta'][:6])
    for row in (0, 5): assert np.array_equal(templ[row], clean[0][row]) and np.array_equal(power[row], clean[1][row])
    # (rows 3 and 4 hold whatever the clamped tables give -- the prior is -inf there; that they index inside the tables is test_phases_under_sanitizers' part)


def test_emulation_refusals():
    """What dl_create refuses (dl_host.hpp::dl_build_obs is the same code), with the library's messages."""
    g, cfg = wsu.load_fixture('kaiser')
    theta = g['theta'][:1]

    def refused(**changes):
        bad = dict(cfg)
        bad.update({'obs0.' + key: value for key, value in changes.items()})
        with pytest.raises(RuntimeError) as info:
            wsu.emulate(bad, theta)
        return str(info.value)

    k = cfg['obs0.ws_k'].copy(); k[900:] *= 1.001
    assert 'must be uniform in log k' in refused(ws_k=k)
    assert 'at least 128 knots' in refused(ws_k=cfg['obs0.ws_k'][::16], ws_pknow=cfg['obs0.ws_pknow'][::16])
    assert 'quadrature' in refused(ws_k=cfg['obs0.ws_k'][:-600], ws_pknow=cfg['obs0.ws_pknow'][:-600])
    kt = np.geomspace(1e-5, 1., len(cfg['obs0.k_t']))
    assert 'template knot' in refused(k_t=kt)
    assert 'outside the fiducial table' in refused(ws_kfid=cfg['obs0.ws_kfid'][100:], ws_pk_tt_fid=cfg['obs0.ws_pk_tt_fid'][100:], ws_pknow_tt_fid=cfg['obs0.ws_pknow_tt_fid'][100:])
    assert 'Kaiser / EFT-like Kaiser / Simple theories only' in refused(theory=np.array([2], dtype='i4'), pknow_dd_fid=cfg['obs0.pk_dd_fid'])
    assert 'ws_kernel' in refused(ws_kernel=np.array([2], dtype='i4'))
    wsu.emulate(cfg, theta)      # the good configuration still goes through


def test_phases_under_sanitizers(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: rows of the fixture with the other knot count (1780) and of 'kaiser', plus
    rows with qbao = 0.3 and 5.0, which must index inside the tables; exit status 0, no report.  (Host code only: nothing sanitized is loaded into this process.)"""
    program = wsu.build_standalone()
    for name in ['tophat_eft', 'kaiser']:
        g, cfg = wsu.load_fixture(name)
        theta = g['theta'][:12].copy()
        iq = [str(n) for n in g['names']].index('qbao')
        theta[6, iq], theta[7, iq] = 0.3, 5.
        fn = os.path.join(str(tmp_path), 'spec_{}.bin'.format(name))
        wsu.write_flat_spec(fn, cfg, theta)
        result = subprocess.run([program, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert result.returncode == 0, result.stderr[-2000:]
        assert 'Sanitizer' not in result.stderr and 'runtime error' not in result.stderr, result.stderr[-2000:]
        assert 'ran inside their tables' in result.stdout


def test_header_documents_the_keys():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'desilike_amd.h')).read()
    assert 'DL_TEMPLATE_WIGGLESPLIT 5' in header
    for key in ['"in.qbao"', '"ws_k"', '"ws_pknow"', '"ws_kfid"', '"ws_pk_tt_fid"', '"ws_pknow_tt_fid"', '"ws_r"', '"ws_kernel"', '"ws_kp"', '"ws_fsigmar_fid"']:
        assert key in header, key
