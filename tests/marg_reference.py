"""Extended-precision restatement of the analytic marginalisation / best fit of linear parameters (likelihoods/base.py:129-200, 314-413): the reference of
tests/test_marg_reference.py (CPU) and tests/test_gpu_marg_counts.py (GPU).  Same inputs and outputs as ``oracle.np_oracle.solve_marginalized``.

The float64 inputs are taken EXACTLY.  The only large sums are the entries of the Gram matrix G = X P X^T of X = [Delta; T_1 .. T_ns] (up to 17 x 512 x 512 products):
every float64 is an integer times a power of two, so these sums are computed in exact integer arithmetic (``exact=True``, the default: a few 0.1 s at n = 512) or term by term in mpmath
(``exact=False``: the same numbers to the working precision, 20 times slower; tests/test_marg_reference.py compares the two).  Everything after G -- the (ns x ns) solve, the quadratic
forms, the log-determinant of the marginalised sub-block -- runs in mpmath at 50 digits and is rounded to float64 once, at the end."""
import numpy as np
import mpmath

DPS = 50


def exact_ints(a):
    """float64 array -> (object array of Python ints I, exponent e) with a == I * 2**e exactly."""
    a = np.asarray(a, dtype='f8')
    if not np.isfinite(a).all(): raise ValueError('marg_reference: non-finite input')
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype('i8')          # |m| < 1: exact 53-bit integers
    e = e.astype('i8') - 53
    nonzero = a != 0.
    emin = int(e[nonzero].min()) if nonzero.any() else 0
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, (mm, ee) in enumerate(zip(mi.reshape(-1).tolist(), e.reshape(-1).tolist())):
        flat[i] = (mm << (ee - emin)) if mm else 0
    return out, emin


def marg_gram(flatdiff, flatderiv, precision, exact=True):
    """G [1 + ns, 1 + ns] = X P X^T (mpmath matrix) of X = [flatdiff; flatderiv]; ``precision`` [n, n], [n] or the output of ``exact_ints`` of either (to convert it once)."""
    X = np.vstack([np.asarray(flatdiff, dtype='f8')[None, :], np.atleast_2d(np.asarray(flatderiv, dtype='f8'))])
    nr = len(X)
    with mpmath.workdps(DPS):
        G = mpmath.zeros(nr, nr)
        if exact:
            Pi, ep = precision if isinstance(precision, tuple) else exact_ints(precision)
            Xi, ex = exact_ints(X)
            Y = Xi * Pi if Pi.ndim == 1 else Xi.dot(Pi)
            Gi = Y.dot(Xi.T)
            for i in range(nr):
                for j in range(nr):
                    G[i, j] = mpmath.ldexp(mpmath.mpf(int(Gi[i, j])), 2 * ex + ep)
        else:
            precision = np.asarray(precision, dtype='f8')
            Xm = [[mpmath.mpf(float(v)) for v in row] for row in X]
            if precision.ndim == 1:
                Y = [[x * mpmath.mpf(float(p)) for x, p in zip(row, precision)] for row in Xm]
            else:
                cols = [[mpmath.mpf(float(v)) for v in col] for col in precision.T]
                Y = [[mpmath.fdot(row, col) for col in cols] for row in Xm]
            for i in range(nr):
                for j in range(nr):
                    G[i, j] = mpmath.fdot(Y[i], Xm[j])
    return G


def marg_from_gram(G, x0, prior_loc, prior_scale, marg_mask):
    """The solve on a Gram matrix of ``marg_gram`` (several prior / '.marg' patterns share one G)."""
    x0, prior_loc, prior_scale = (np.atleast_1d(np.asarray(a, dtype='f8')) for a in (x0, prior_loc, prior_scale))
    marg = np.flatnonzero(np.asarray(marg_mask, dtype='?'))
    ns = len(x0)
    assert G.rows == 1 + ns and len(prior_loc) == ns and len(prior_scale) == ns
    with mpmath.workdps(DPS):
        mpf = mpmath.mpf
        prec = [mpf(0) if np.isinf(s) else 1 / mpf(float(s))**2 for s in prior_scale]                        # 181 (flat prior: 0)
        HL = mpmath.matrix(ns, ns)
        for i in range(ns):
            for j in range(ns): HL[i, j] = -G[1 + i, 1 + j]                                                      # 174
        gL = mpmath.matrix([-G[1 + i, 0] for i in range(ns)])                                                    # 173
        H = HL.copy()
        for i in range(ns): H[i, i] -= prec[i]                                                                   # 183-185
        g = mpmath.matrix([gL[i] - (mpf(float(x0[i])) - mpf(float(prior_loc[i]))) * prec[i] for i in range(ns)])   # 182
        dx = -mpmath.lu_solve(H, g)                                                                              # 188
        x = [mpf(float(x0[i])) + dx[i] for i in range(ns)]                                                       # 189
        loglikelihood = -G[0, 0] / 2 + (dx.T * HL * dx)[0] / 2 + (gL.T * dx)[0]                                  # 385-386
        logprior = sum((-(x[i] - mpf(float(prior_loc[i])))**2 * prec[i] / 2 for i in range(ns)), mpf(0))          # 363-364
        if marg.size:                                                                                            # 394-404: no (2 pi)^(n/2)
            sub = mpmath.matrix(marg.size, marg.size)
            for a, i in enumerate(marg):
                for b, j in enumerate(marg): sub[a, b] = -H[int(i), int(j)]
            det = mpmath.det(sub)
            if not det > 0: raise ValueError('marg_reference: the marginalised block of the posterior Hessian is not negative definite')
            loglikelihood -= mpmath.log(det) / 2
        return dict(loglikelihood=float(loglikelihood), logprior_solved=float(logprior), x=np.array([float(v) for v in x]), dx=np.array([float(v) for v in dx]),
                    likelihood_hessian=np.array([[float(HL[i, j]) for j in range(ns)] for i in range(ns)]), chi2_x0=float(G[0, 0]))


def marg_reference(flatdiff, flatderiv, precision, x0, prior_loc, prior_scale, marg_mask, exact=True):
    """One parameter point, arguments of ``oracle.np_oracle.solve_marginalized``: dict(loglikelihood, logprior_solved, x, dx, likelihood_hessian) in float64, and ``chi2_x0``."""
    return marg_from_gram(marg_gram(flatdiff, flatderiv, precision, exact=exact), x0, prior_loc, prior_scale, marg_mask)
