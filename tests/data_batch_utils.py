"""Shared by tests/test_data_batch.py and tests/test_gpu_data_batch.py: builds of the stand-alone CPU program of the data-batch reduction
(tests/csrc/emulate_data_batch.cpp), the configurations of the GPU tests with their data vectors swapped, and the single-data references.  Test infrastructure only."""
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE_FLAGS = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']


def build_program(sanitize=False):
    """tests/csrc/emulate_data_batch.cpp as a program of its own (host code only; nothing of it is loaded into python); ``sanitize``: under ASan + UBSan."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, 'emulate_data_batch_asan' if sanitize else 'emulate_data_batch')
    src = os.path.join(HERE, 'csrc', 'emulate_data_batch.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in ['dl_data_batch.h', 'dl_fullshape.h']]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + (['-O1'] + SANITIZE_FLAGS if sanitize else ['-O2']) + ['-o', out, src])
    return out


# ---- configurations ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """One configuration: ``spec`` (nested golden spec or flat reference-side keys), its own data vector, theta rows inside the priors, the precision and the priors."""

    def __init__(self, name):
        from golden_utils import load_golden, spec_from_golden, spec_from_golden_bao
        self.name = name
        if name.startswith('boundary_'):
            from test_gpu_boundary import load_fixture
            g, cfg = load_fixture(name[len('boundary_'):])
            self.flat, self.spec = True, {key: np.array(value) for key, value in cfg.items()}
            self.n_obs = int(np.ravel(cfg['n_obs'])[0])
            self.flatdata = np.concatenate([np.ravel(cfg['obs{:d}.flatdata'.format(i)]).astype('f8') for i in range(self.n_obs)])
            self.priors = np.reshape(cfg['priors'], (-1, 5)).astype('f8')
            precision = np.asarray(cfg['precision'], dtype='f8')
            theta = np.asarray(g['theta'], dtype='f8')
            self.g = None
        else:
            g = load_golden(name)
            self.g = g
            self.flat, self.spec = False, (spec_from_golden_bao(g) if name.startswith('cfg4_bao') else spec_from_golden(g))
            self.n_obs = len(self.spec['observables'])
            self.flatdata = np.concatenate([np.ravel(obs['flatdata']).astype('f8') for obs in self.spec['observables']])
            self.priors = np.reshape(g['priors'], (-1, 5)).astype('f8')
            precision = np.asarray(g['precision'], dtype='f8')
            theta = np.asarray(g['theta'], dtype='f8')
        n = self.flatdata.size
        self.precision = precision if precision.size == n else precision.reshape(n, n)
        inside = ((theta >= self.priors[:, 1]) & (theta <= self.priors[:, 2])).all(axis=1) & np.isfinite(theta).all(axis=1)
        self.theta_inside = theta[inside]
        assert len(self.theta_inside) >= 2, name

    def sizes(self):
        if self.flat: return [np.size(self.spec['obs{:d}.flatdata'.format(i)]) for i in range(self.n_obs)]
        return [np.size(obs['flatdata']) for obs in self.spec['observables']]

    def spec_with_data(self, flatdata):
        """The configuration with its data vector replaced (``obs<i>.flatdata``)."""
        blocks = np.split(np.asarray(flatdata, dtype='f8'), np.cumsum(self.sizes())[:-1])
        if self.flat:
            spec = dict(self.spec)
            for i, block in enumerate(blocks): spec['obs{:d}.flatdata'.format(i)] = block.copy()
            return spec
        spec = dict(self.spec)
        spec['observables'] = [dict(obs, flatdata=block.copy()) for obs, block in zip(self.spec['observables'], blocks)]
        return spec

    def mocks(self, M, seed=5):
        """``flatdata + 0.05 |flatdata| z``, z seeded standard normal: [M, n]."""
        z = np.random.RandomState(seed).standard_normal((M, self.flatdata.size))
        return self.flatdata + 0.05 * np.abs(self.flatdata) * z

    def points(self, B, seed=9):
        """B points inside the priors: convex combinations of two of the fixture's rows inside them (the priors are boxes)."""
        rng = np.random.RandomState(seed)
        rows = self.theta_inside
        i, j, a = rng.randint(len(rows), size=B), rng.randint(len(rows), size=B), rng.uniform(size=(B, 1))
        return np.ascontiguousarray(a * rows[i] + (1. - a) * rows[j])

    def oracle_logprior(self, theta):
        from oracle import np_oracle as orc
        priors = [dict(dist=['uniform', 'norm'][int(row[0])], limits=(row[1], row[2]), loc=row[3], scale=row[4]) for row in self.priors]
        return orc.logprior(theta, priors)

    def oracle_flattheory(self, row):
        """flattheory of one point by oracle/np_oracle.py where it evaluates the configuration from the fixture (the Kaiser full-shape ones); None elsewhere."""
        if self.g is None or self.name.startswith('cfg4_bao'): return None
        from golden_utils import observable_constants
        from oracle import np_oracle as orc
        names = [str(n) for n in self.g['names']]
        p = dict(zip(names, row))
        out = []
        for iobs in range(self.n_obs):
            c = observable_constants(self.g, iobs)
            prefix = str(c['tracer']) + '.' if str(c.get('tracer', '')) else ''
            out.append(orc.fullshape_observable(c, dict(p, b1=(p[prefix + 'b1'],) * 2, sn0=p[prefix + 'sn0']))['flattheory'])
        return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def get_case(name):
    return Case(name)


MMAX, BMAX = 65, 300


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, mocks [MMAX, n], theta [BMAX, P], ref [BMAX, MMAX], flattheory [BMAX, n]): the log-posteriors of the project's single-data path -- one context per data
    vector, created from the same configuration with its data replaced, evaluated with dl_eval_logposterior -- computed once and shared by the tests."""
    from desilike_amd._lib import Context
    case = get_case(name)
    mocks, theta = case.mocks(MMAX), case.points(BMAX)
    ref = np.empty((BMAX, MMAX))
    flattheory = None
    for m in range(MMAX):
        ctx = Context(case.spec_with_data(mocks[m]), device=0)
        ref[:, m], status = ctx.eval_logposterior_host(theta)
        assert (status == 0).all()
        if m == 0: flattheory = ctx.eval_batch_host(theta, return_flattheory=True)[3]
        ctx.close()
    ref.setflags(write=False); mocks.setflags(write=False); theta.setflags(write=False); flattheory.setflags(write=False)
    return case, mocks, theta, ref, flattheory
