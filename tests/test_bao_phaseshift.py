"""CPU: the BAO phase-shift template (reference: power_template.py:442-496) -- the NumPy / scipy oracle against fixtures captured from the reference
(tests/golden/make_phaseshift_fixture.py), the mirror class against the reference's parameter file, and the new device phases of the BAO kernel (csrc/dl_fullshape.h,
``dl_bao_ps_*``) run on the CPU (tests/csrc/emulate_phaseshift.cpp): as a shared object against the fixtures, and as a program of its own under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as orc
import phaseshift_oracle as pso
import phaseshift_utils as psu


@pytest.mark.parametrize('name', psu.FIXTURES)
def test_oracle_vs_reference(name):
    """Tolerances of tests/test_oracle_bao.py for the cfg4 fixtures."""
    g, cfg = psu.load_fixture(name)
    assert g['theta'].shape[0] == 48
    ishift = [str(n) for n in g['names']].index('baoshift')
    assert tuple(g['theta'][:3, ishift]) == (-8., 1., 10.)
    for i in range(48):
        row, ref = g['theta'][i], g['wiggle_power'][i]
        flat, powers = pso.flattheory(cfg, row)
        power = np.concatenate([np.ravel(p) for p in powers])
        assert np.allclose(power, ref, rtol=1e-11, atol=1e-12 * np.abs(ref).max())
        assert np.allclose(flat, g['flattheory'][i], rtol=1e-11, atol=1e-13 * np.abs(g['flattheory'][i]).max())
        logl = orc.gaussian_loglikelihood(flat, pso.flatdata(cfg), pso.precision(cfg))[0]
        assert abs(logl - g['loglikelihood'][i]) <= 1e-10 * max(1., abs(g['loglikelihood'][i]))


def test_fixture_clip_is_live():
    """The cases the fixtures are there for: the lower clip at baoshift = -8 (and, with the template starting at 1e-4 below the inner grid, at every point of 'clip' with baoshift <= 1), the upper
    clip at baoshift = 10 of 'clip' only."""
    for name, upper in [('pk', False), ('clip', True)]:
        g, cfg = psu.load_fixture(name)
        c = pso.observable_keys(cfg)
        ishift = [str(n) for n in g['names']].index('baoshift')
        shifted = c['k_t'][None, :] + (g['theta'][:, ishift, None] - 1.) * c['ps_kshift'][None, :]
        assert (shifted[0] < 0.).sum() > 400 and (shifted[0] < c['ps_klim'][0]).any()
        assert (shifted[2] > c['ps_klim'][1]).any() == upper
        if upper: assert (shifted < c['ps_klim'][0]).any(axis=1)[g['theta'][:, ishift] <= 1.].all()


def test_no_shortcut_at_baoshift_one():
    """baoshift = 1 is NOT the plain BAO template: the wiggles pass through the inner spline from the other grid (a few 1e-11 of the template, above the theory tolerance)."""
    g, cfg = psu.load_fixture('pk')
    c = pso.observable_keys(cfg)
    plain, shifted = c['pk_dd_fid'], pso.pk_dd(c, 1.)
    assert np.allclose(shifted, plain, rtol=1e-9) and np.abs(shifted / plain - 1.).max() > 1e-12


def test_mirror_parameters_match_reference():
    from desilike_amd.theories.galaxy_clustering import BAOPhaseShiftPowerSpectrumTemplate, BAOPowerSpectrumTemplate
    assert issubclass(BAOPhaseShiftPowerSpectrumTemplate, BAOPowerSpectrumTemplate)
    for name, apnames in [('pk', ['qpar', 'qper']), ('clip', ['qiso'])]:
        g, like = psu.make_likelihood(name)
        assert like.varied_params.names() == [str(n) for n in g['names']]
        limits = np.array([like.varied_params[n].prior.limits for n in like.varied_params.names()], dtype='f8')
        assert np.array_equal(limits, g['prior_limits'])
        template = like.observables[0].wmatrix.theory.template
        ref = {str(n): i for i, n in enumerate(g['params/names'])}
        mine = [param for param in template.params]
        assert [param.basename for param in mine] == apnames + ['baoshift']                     # the AP parameters of the apmode, then baoshift
        assert [ref[param.basename] for param in mine] == sorted(ref[param.basename] for param in mine)   # ... in the reference's order
        for param in mine:
            i = ref[param.basename]
            assert param.value == g['params/value'][i] and not param.fixed and not g['params/fixed'][i]
            assert tuple(param.prior.limits) == tuple(g['params/prior_limits'][i]) and tuple(param.ref.limits) == tuple(g['params/ref_limits'][i])
            assert param.delta[0] == param.value and param.delta[1] == param.delta[2] == g['params/delta'][i]      # (centre, step below, step above)
            assert param.latex() == str(g['params/latex'][i])
    baoshift = template.params['baoshift']
    assert baoshift.value == 1. and tuple(baoshift.prior.limits) == (-8., 10.) and baoshift.delta[1:] == (8., 8.)
    assert (template.phiinf, template.kstar, template.epsilon, template.with_now) == (0.227, 0.0324, 0.872, 'peakaverage')
    # the constants the kernel receives are the reference's own, to the last bit
    g, cfg = psu.load_fixture('clip')
    spec = like._spec({}, like._flatdata_list(), like.precision)['observables'][0]
    for key in ['k_t', 'pknow_dd_fid', 'ps_kshift', 'ps_k', 'ps_wiggles', 'ps_klim', 'template', 'theory', 'bao_mode']:
        assert np.array_equal(np.ravel(spec[key]), np.ravel(cfg['obs0.' + key])), key
    assert tuple(spec['inputs']['baoshift']) == tuple(cfg['obs0.in.baoshift'])


def test_mirror_routing_and_refusals():
    from desilike_amd.fiducial import TabulatedFiducial, SyntheticFiducial
    from desilike_amd.theories.galaxy_clustering import (BAOPhaseShiftPowerSpectrumTemplate, DampedBAOWigglesTracerPowerSpectrumMultipoles, KaiserTracerPowerSpectrumMultipoles,
                                                         TNSTracerPowerSpectrumMultipoles, PNGTracerPowerSpectrumMultipoles, ResummedBAOWigglesTracerCorrelationFunctionMultipoles,
                                                         SimpleBAOWigglesTracerPowerSpectrumMultipoles, FlexibleBAOWigglesTracerPowerSpectrumMultipoles)
    # only_now: the wiggles are identically zero (power_template.py:493-495) -- the plain BAO template on the no-wiggle table, no baoshift input
    theory = DampedBAOWigglesTracerPowerSpectrumMultipoles(template=BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial='synthetic', only_now=True))
    spec = theory._theory_spec()
    assert int(spec['template'][0]) == 0 and 'ps_k' not in spec and 'baoshift' not in theory._input_map()
    assert np.array_equal(spec['pk_dd_fid'], spec['pknow_dd_fid'])
    # every BAO wiggle theory takes the template
    for cls in [SimpleBAOWigglesTracerPowerSpectrumMultipoles, FlexibleBAOWigglesTracerPowerSpectrumMultipoles, ResummedBAOWigglesTracerCorrelationFunctionMultipoles]:
        theory = cls(template=BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial='synthetic'))
        spec = theory._theory_spec()
        assert int(spec['template'][0]) == 4 and theory._input_map()['baoshift'] == 'baoshift' and len(spec['ps_wiggles']) == 2000
    # ... and the others name what is supported
    for cls in [KaiserTracerPowerSpectrumMultipoles, TNSTracerPowerSpectrumMultipoles, PNGTracerPowerSpectrumMultipoles]:
        with pytest.raises(NotImplementedError, match='BAOWigglesTracer'):
            cls(template=BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial='synthetic')).initialize()
    # inner grid: the ends of a tabulated fiducial's own table; rs_drag is needed
    fid = SyntheticFiducial()
    k = np.geomspace(5e-5, 20., 600)
    tabulated = dict(k=k, pk_dd=fid.pk_dd(k), pknow_dd=fid.pknow_dd(k), f=0.8)
    template = BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial=TabulatedFiducial(rs_drag=100., **tabulated))
    DampedBAOWigglesTracerPowerSpectrumMultipoles(template=template).initialize()
    assert template.klim_wiggles == (k[0], k[-1]) and template.k_wiggles.size == 2000
    template = BAOPhaseShiftPowerSpectrumTemplate(z=0.5, fiducial=TabulatedFiducial(**tabulated))
    for attempt in range(2):      # (the second call raises again: the template is not left half initialised)
        with pytest.raises(ValueError, match='rs_drag'):
            DampedBAOWigglesTracerPowerSpectrumMultipoles(template=template).initialize()
        assert not hasattr(template, 'kshift')


@pytest.mark.parametrize('name', psu.FIXTURES)
def test_phase_emulation_vs_reference(name):
    """The device phase functions on the CPU, all 48 points with 64 / 128 / 192 / 256 emulated threads per point (what dl_bao_threads gives: 64 and 128 by the batch; below,
    the wavenumbers rounded up to whole waves -- 192 for the 168 of the P_ell fixtures, 256 for the 300 of 'xi'): the bound of tests/test_gpu_bao.py:21."""
    g, cfg = psu.load_fixture(name)
    ref = g['wiggle_power']
    for nthr in (64, 128, 192, 256):
        power = psu.emulate_wiggle_power(cfg, g['theta'], nthr)
        assert np.allclose(power, ref, rtol=1e-11, atol=1e-12 * np.abs(ref).max()), nthr


def test_phase_emulation_nan_baoshift():
    """A NaN baoshift gives NaN multipoles, as np.clip in the reference does (power_template.py:491) -- not the finite wiggle of a wavenumber clipped to the lower bound."""
    g, cfg = psu.load_fixture('pk')
    theta = g['theta'][:2].copy()
    theta[1, [str(n) for n in g['names']].index('baoshift')] = np.nan
    power = psu.emulate_wiggle_power(cfg, theta, 64)
    assert np.isfinite(power[0]).all() and np.isnan(power[1]).all()
    assert np.isnan(pso.shifted_wiggles(pso.observable_keys(cfg), np.nan)).all()


def test_emulation_refusals():
    """What dl_create refuses (dl_host.hpp::dl_build_obs is the same code): the kind on another theory, template knots that are not uniform, an inner grid that is not uniform."""
    g, cfg = psu.load_fixture('pk')
    theta = g['theta'][:1]

    def refused(**changes):
        bad = dict(cfg)
        bad.update({'obs0.' + key: value for key, value in changes.items()})
        with pytest.raises(RuntimeError) as info:
            psu.emulate_wiggle_power(bad, theta, 64)
        return str(info.value)

    kt = cfg['obs0.k_t'].copy(); kt[1000] *= 1. + 1e-9
    assert 'uniform' in refused(k_t=kt)
    kw = cfg['obs0.ps_k'].copy(); kw[500:] *= 1.001
    assert 'uniform' in refused(ps_k=kw)
    assert 'BAO wiggle theories only' in refused(theory=np.array([0], dtype='i4'))
    assert 'ps_kshift' in refused(ps_kshift=cfg['obs0.ps_kshift'][:-1])


def test_phases_under_sanitizers(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: all 48 points of the fixture with the live upper clip, 64, 128, 192 and 256
    emulated threads; exit status 0, no report.  (Host code only: nothing sanitized is loaded into this process.)"""
    program = psu.build_standalone()
    g, cfg = psu.load_fixture('clip')
    fn = os.path.join(str(tmp_path), 'spec.bin')
    psu.write_flat_spec(fn, cfg, g['theta'])
    result = subprocess.run([program, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode == 0, result.stderr[-2000:]
    assert 'Sanitizer' not in result.stderr and 'runtime error' not in result.stderr, result.stderr[-2000:]
    assert '64 / 128 / 192 / 256 threads agree' in result.stdout


@pytest.mark.parametrize('name', psu.FIXTURES)
def test_reference_side_keys_are_documented(name):
    """Every key extract_config emits for the template is one include/desilike_amd.h documents (as tests/test_gpu_boundary.py checks for the other fixtures)."""
    import re
    header = open(os.path.join(psu.HERE, '..', 'include', 'desilike_amd.h')).read()
    g, cfg = psu.load_fixture(name)
    assert int(cfg['obs0.template'][0]) == 4 and 'DL_TEMPLATE_PHASESHIFT 4' in header
    lines = header.split('\n')
    generic = set(lines[[i for i, line in enumerate(lines) if 'obs<i>.in.<name>' in line][0] + 1].replace('*', ' ').split())     # the inputs listed by bare name under 'obs<i>.in.<name>'
    assert 'qpar' in generic and 'df' in generic
    for key in cfg:           # every key as a whole word of the header; an input as 'in.<name>' or in the list of generic inputs
        tail = re.sub(r'^obs\d+\.', '', key)
        assert re.search(r'(?<![A-Za-z0-9_])' + re.escape(tail) + r'(?![A-Za-z0-9_])', header) or (tail.startswith('in.') and tail[3:] in generic), key
    for key in ['"in.baoshift"', '"ps_kshift"', '"ps_k"', '"ps_wiggles"', '"ps_klim"']:
        assert key in header, key
