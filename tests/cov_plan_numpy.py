"""NumPy replay of ``dl_cov_kernel`` and ``dl_cov_sym_kernel`` (csrc/dl_cov.hip) on the host arrays of ``CovariancePlanBuilder.arrays()``: the same reads, the same
operations in the same order per cell (without the FMA contraction the device compiler is free to apply).  It separates "the builder lists the wrong cells", which any
CPU shows against the oracle (tests/test_cov_cases.py), from "the kernel reads them wrongly" (tests/test_gpu_cov_shapes.py).

The keyword arguments plant the errors tests/test_cov_cases.py uses to show that the comparison has teeth."""
import numpy as np

MAX_ELLS = 5        # DL_COV_MAX_ELLS


def apply_plan(arrays, ell0, shotnoise, powers, symmetrise=True, drop_last_point=False, ignore_ell0=False, magnitude=False):
    """``arrays``: dict of ``CovariancePlanBuilder.arrays()``; ``ell0`` / ``shotnoise``: per theory, index of the monopole among its multipoles (or -1) and shot
    noise; ``powers``: per theory [n_ell, n_k].  Returns the covariance [n, n].

    Planted errors: ``drop_last_point`` loses the last integration point of every cell, ``ignore_ell0`` takes the first multipole of every theory for the monopole,
    ``symmetrise=False`` skips ``dl_cov_sym_kernel``.

    ``magnitude=True``: the same sums with every term replaced by its absolute value (|I|, |w2|, the zero lag added instead of removed, |front|, |const|): the size of
    what each element is a sum of, which a rounding-error bound scales with (:func:`rounding_bound`)."""
    n = int(arrays['n'])
    cell_i, cell_d, pt_i, pt_d, gtab = arrays['cell_i'], arrays['cell_d'], arrays['pt_i'], arrays['pt_d'], arrays['gtab']
    powers = [np.asarray(power, dtype='f8') for power in powers]
    ell0 = [0 if ignore_ell0 else int(e) for e in ell0]
    cov = np.zeros((n, n), dtype='f8')                         # hipMemsetAsync: the cells no block lists stay 0
    # cells grouped by their pair of theories: the multipole loops then have fixed bounds
    pairs = sorted(set((int(t1), int(t2)) for t1, t2 in cell_i[:, 2:4]))
    for t1, t2 in pairs:
        cells = np.flatnonzero((cell_i[:, 2] == t1) & (cell_i[:, 3] == t2))
        P1, P2, e1, e2, sn1, sn2 = powers[t1], powers[t2], ell0[t1], ell0[t2], float(shotnoise[t1]), float(shotnoise[t2])
        n1, n2 = P1.shape[0], P2.shape[0]
        assert n1 <= MAX_ELLS and n2 <= MAX_ELLS
        first, count = cell_i[cells, 6].astype(np.int64), cell_i[cells, 7].astype(np.int64)
        if drop_last_point: count = np.maximum(count - 1, 0)
        zero_lag = cell_i[cells, 5] != 0
        G = gtab[cell_i[cells, 4]]                             # [cells, 5, 5]
        if magnitude: G = np.abs(G)
        total = np.zeros(cells.size)
        for step in range(int(count.max()) if cells.size else 0):            # sum over q in the order of the kernel's loop, all cells of the pair at once
            live = np.flatnonzero(step < count)
            q = first[live] + step
            j1, j2 = pt_i[q, 0], pt_i[q, 1]
            a1, h1, a2, h2, w, w2 = pt_d[q].T
            if magnitude: w, w2 = np.abs(w), np.abs(w2)
            p2 = []
            fabs = np.abs if magnitude else (lambda v: v)
            for lb in range(n2):
                f0, f1 = P2[lb, j2] + (sn2 if lb == e2 else 0.), P2[lb, j2 + 1] + (sn2 if lb == e2 else 0.)
                p2.append(fabs(((f1 - f0) / h2) * a2 + f0))
            sigma = np.zeros(live.size)
            for la in range(n1):
                f0, f1 = P1[la, j1] + (sn1 if la == e1 else 0.), P1[la, j1 + 1] + (sn1 if la == e1 else 0.)
                p1 = fabs(((f1 - f0) / h1) * a1 + f0)
                for lb in range(n2):
                    lag = np.where(zero_lag[live], sn1 * sn2, 0.) if (la == e1 and lb == e2) else 0.
                    sigma = sigma + (p1 * p2[lb] + lag if magnitude else p1 * p2[lb] - lag) * G[live, la, lb]
            sigma = (np.abs(cell_d[cells[live], 0]) if magnitude else cell_d[cells[live], 0]) * sigma
            total[live] = total[live] + (sigma * w) * w2
        if magnitude: cov[cell_i[cells, 0], cell_i[cells, 1]] = np.abs(cell_d[cells, 1]) * total / np.abs(cell_d[cells, 2]) + np.abs(cell_d[cells, 3])
        else: cov[cell_i[cells, 0], cell_i[cells, 1]] = cell_d[cells, 1] * total / cell_d[cells, 2] + cell_d[cells, 3]
    if symmetrise:
        for r, c in arrays['sym']:
            cov[r, c] = cov[c, r] = (cov[r, c] + cov[c, r]) / 2.
    return cov


def rounding_bound(arrays, ell0, shotnoise, powers):
    """Element-wise bound on the distance between two correct evaluations of the plan that differ only in where they round (the device compiler contracts a * b + c
    into one FMA; this replay rounds twice): every rounding moves a partial result by at most half an ulp (2^-53) of its size, at most the absolute sum
    ``apply_plan(magnitude=True)``; per integration point there are 4 roundings per interpolated multipole (at most 2 x 5), 3 per pair of multipoles (at most 25) and 4
    for the weights, then one addition per point, and 4 operations after the loop and in the symmetrisation:

        |difference| <= (99 + Q + 4) 2^-53 magnitude,    Q = the largest number of points of a cell.

    A worst-case bound from the operation count alone: nothing in it comes from the kernel's output."""
    Q = int(arrays['cell_i'][:, 7].max()) if len(arrays['cell_i']) else 0
    return (99 + Q + 4) * 2.**-53 * apply_plan(arrays, ell0, shotnoise, powers, magnitude=True)
