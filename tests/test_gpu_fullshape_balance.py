"""GPU (-m gpu): the raised priority of the mu wave in the fast full-shape theory kernels (csrc/dl_kernels.hip: dl_fullshape_body, ``s_setprio`` on the wave that runs
the per-mu chain, from entry to the barrier before the evaluation phase).  A scheduling hint may not change a bit of any result: the default path is compared bit for bit
with ``DL_FS_MU_PRIO=0`` (a child process computes every case once and hands the arrays back in an ``.npz``: the switch is read once per process), and against the NumPy
oracle at the suite's 1e-10 on log-likelihoods (relative above 1).

Cases: BASELINE configs[1] (multipoles (0, 2, 4) x 400 wavenumbers) at 257, 1000 and 1024 points -- batches of 256 or fewer take the 512-thread form, 1024 points put
four workgroups on every CU; the two-tracer configs[4] likelihood at 512 points (grid y = 2: the launch for several observables) and as a 512-walker device-resident
ensemble (the folded launch); and two small likelihoods, multipoles (0, 2) and (0, 2, 4, 6, 8) (both instantiations of the kernels), at 261 points (256-thread form) and 37
points (512-thread form)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path[:0] = [d for d in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),) if d not in sys.path]   # (the child process is started as a script)

import bench   # noqa: E402  (the generators of configs[1] and configs[4])
from oracle import np_oracle as orc   # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = {'no-priority': dict(DL_FS_MU_PRIO='0')}
BATCHES = (257, 1000, 1024)
# name: multipoles, wavenumbers
SMALL = {'l02-k400': ((0, 2), 400), 'l02468-k280': ((0, 2, 4, 6, 8), 280)}
SMALL_BATCHES = (37, 261)


def build_small(ells, nk, seed=4):
    """One observable with a random dense window that reaches every input wavenumber"""
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    rng = np.random.RandomState(seed)
    kout = np.arange(0.025, 0.33, 0.02)
    kin = np.linspace(5e-4, 0.35, nk)
    nout = len(ells) * len(kout)
    wmat = np.abs(rng.standard_normal((nout, len(ells) * nk))) * 0.02
    for ill in range(len(ells)):
        for i, kk in enumerate(kout):
            wmat[ill * len(kout) + i, ill * nk + np.argmin(np.abs(kin - kk))] += 1.
    wmat /= wmat.sum(axis=1)[:, None]
    theory = KaiserTracerPowerSpectrumMultipoles(template=ShapeFitPowerSpectrumTemplate(z=0.8))
    obs = TracerPowerSpectrumMultipolesObservable(data={'b1': 1.7}, k=kout, ells=ells, wmatrix=wmat, kin=kin, ellsin=ells, theory=theory, shotnoise=2e3)
    A = rng.standard_normal((nout, nout)) * 15.
    like = ObservablesGaussianLikelihood(observables=[obs], covariance=A.dot(A.T) + 1e4 * np.eye(nout))
    like.initialize()
    return like


def small_points(like, n, seed=11):
    """n rows: AP and shape parameters over their whole prior ranges, the others around their values"""
    rng = np.random.RandomState(seed)
    params = list(like.varied_params)
    lo, hi = np.array([param.prior.limits[0] for param in params]), np.array([param.prior.limits[1] for param in params])
    ref = np.array([param.value for param in params])
    wide = np.array([param.name in ('qpar', 'qper', 'dm') for param in params])
    return np.where(wide, rng.uniform(np.where(wide, lo, 0.), np.where(wide, hi, 1.), size=(n, len(params))),
                    ref * rng.uniform(0.9, 1.1, size=(n, len(params))) + rng.uniform(-0.05, 0.05, size=(n, len(params))))


class Cases:
    """The likelihoods and their points, built once per process"""
    cache = {}

    @classmethod
    def get(cls, name):
        if name not in cls.cache:
            if name == 'cfg1':
                like = bench.make_likelihood(0)
                theta = bench.sample_theta(like, max(BATCHES), seed=42)
            elif name == 'cfg5':
                like = bench.make_likelihood_config5(0)
                theta = bench.sample_theta(like, 512, seed=43)
            else:
                like = build_small(*SMALL[name])
                theta = small_points(like, max(SMALL_BATCHES))
            cls.cache[name] = (like, np.ascontiguousarray(theta))
        return cls.cache[name]


def gpu_outputs():
    """Everything the settings are compared on, as {key: array}"""
    out = {}

    def batch(name, B):
        like, theta = Cases.get(name)
        ctx = like._get_context()
        for key, value in zip(['loglike', 'logprior', 'status', 'flattheory'], ctx.eval_batch_host(theta[:B], return_flattheory=True)):
            out['{}/{:d}/{}'.format(name, B, key)] = value
        pctx, offset = like._get_posterior_context()
        out['{}/{:d}/logposterior'.format(name, B)] = pctx.eval_logposterior_host(theta[:B])[0]
        for iobs in range(len(like.observables)):
            out['{}/{:d}/power{:d}'.format(name, B, iobs)] = ctx.eval_theory_host(theta[:B], iobs=iobs)    # rows of n_in doubles: the other row stride

    for B in BATCHES: batch('cfg1', B)
    batch('cfg5', 512)
    for name in SMALL:
        for B in SMALL_BATCHES: batch(name, B)
    from desilike_amd.samplers import EmceeSampler
    sampler = EmceeSampler(Cases.get('cfg5')[0], nwalkers=512, seed=42, device_resident=True)
    sampler.run(niterations=6)
    out['ensemble/coords'], out['ensemble/logposterior'] = (np.asarray(a) for a in sampler._last)
    return out


def oracle_loglike(like, theta):
    consts, bias_names = [], []
    for obs in like.observables:
        wm, theory = obs.wmatrix, obs.wmatrix.theory
        tpl = theory.template
        consts.append(dict(template='shapefit', k11=tpl.k, pk_dd_fid=tpl.pk_dd_fid, f_fid=tpl.f_fid, kp=tpl.kp, a=tpl.a, kin=theory.k, mu=theory.mu, wmu_ell=theory.wmu,
                           ellsin=theory.ells, nd=theory.nd, matrix_full=wm.matrix_full, kmask=getattr(wm, 'kmask', None), offset=getattr(wm, 'offset', None),
                           shotnoisein=wm.shotnoisein, shotnoiseout=wm.shotnoiseout, flatdata=obs.flatdata))
        if consts[-1]['kmask'] is None: del consts[-1]['kmask'], consts[-1]['offset']
        bias_names.append(theory._bias_names())
    names = like.varied_params.names()
    flatdata = np.concatenate(like._flatdata_list())
    ref = np.empty(len(theta))
    for i, row in enumerate(theta):
        p = dict(zip(names, row))
        flat = []
        for c, bias in zip(consts, bias_names):
            q = {name: p[name] for name in ['qpar', 'qper', 'dm', 'df'] if name in p}
            q['b1'] = (p[bias['b1X']], p[bias['b1Y']])
            q['sn0'] = p[bias['sn0']]
            flat.append(orc.fullshape_observable(c, q)['flattheory'])
        ref[i] = orc.gaussian_loglikelihood(np.concatenate(flat), flatdata, like.precision)[0]
    return ref


@pytest.fixture(scope='module')
def default_outputs():
    return gpu_outputs()


@pytest.fixture(scope='module')
def switched_outputs():
    """One child process per setting (the switch is read once per process)"""
    with tempfile.TemporaryDirectory() as tmp:
        children = {}
        for name, env in SWITCHES.items():
            fn = os.path.join(tmp, name + '.npz')
            children[name] = (fn, subprocess.Popen([sys.executable, os.path.abspath(__file__), fn], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE))
        outputs = {}
        for name, (fn, child) in children.items():
            stdout, stderr = child.communicate(timeout=600)
            assert child.returncode == 0 and 'every case written' in stdout.decode(), (name, stderr.decode()[-2000:])
            with np.load(fn) as f: outputs[name] = {key: f[key] for key in f.files}
        yield outputs


@pytest.mark.parametrize('setting', list(SWITCHES))
def test_bit_for_bit_against_the_switched_off_path(setting, default_outputs, switched_outputs):
    other = switched_outputs[setting]
    assert sorted(other) == sorted(default_outputs)
    different = [key for key, value in default_outputs.items() if not np.array_equal(value, other[key], equal_nan=True)]
    assert not different, different


@pytest.mark.parametrize('B', BATCHES)
def test_configs1_against_the_oracle(B, default_outputs):
    like, theta = Cases.get('cfg1')
    if 'cfg1' not in oracle_cache: oracle_cache['cfg1'] = oracle_loglike(like, theta)
    check_oracle(default_outputs, 'cfg1', B, oracle_cache['cfg1'][:B])


oracle_cache = {}


def check_oracle(outputs, name, B, ref):
    loglike, status = outputs['{}/{:d}/loglike'.format(name, B)], outputs['{}/{:d}/status'.format(name, B)]
    err = np.abs(loglike - ref) / np.maximum(1., np.abs(ref))
    print('{} batch {:d}: largest log-likelihood error {:.3g}'.format(name, B, err.max()))
    assert (status == 0).all() and (err <= 1e-10).all(), (name, B, float(err.max()))


def test_two_observables_against_the_oracle(default_outputs):
    like, theta = Cases.get('cfg5')
    check_oracle(default_outputs, 'cfg5', 512, oracle_loglike(like, theta))


@pytest.mark.parametrize('name', list(SMALL))
def test_both_instantiations_against_the_oracle(name, default_outputs):
    like, theta = Cases.get(name)
    assert like._get_context().info('moment_form_obs0') == 3      # the moment form is what runs
    ref = oracle_loglike(like, theta)
    for B in SMALL_BATCHES: check_oracle(default_outputs, name, B, ref[:B])


if __name__ == '__main__':
    import warnings
    warnings.simplefilter('ignore')
    np.savez(sys.argv[1], **gpu_outputs())
    print('every case written')
