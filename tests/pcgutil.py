"""Test helper: the preconditioned conjugate gradient loop of the host layer's CGSolver (hyteg_amd/host/solvers.hpp,
solvePreconditioned; src/hyteg/solvers/CGSolver.hpp:94-203 with init() :340-358) restated in numpy on global vectors, and the
forward + backward sweep preconditioner (SymmetricGaussSeidelSmoother / SymmetricSORSmoother) built on
hostutil.GlobalSweepOracle.sweep."""
import math

import numpy as np


def pcg(apply, precond, x0, b, free, max_iter, rel_tol=0.0, abs_tol=0.0):
    """apply(u): A u on a global vector; precond(r): z with M z = r from z = 0 (a global vector, only its `free` entries are used);
    free: boolean mask of the points the solver's flag selects (everything else is boundary data that x keeps).
    Returns (x, iterations, iterates): iterates[i] is x after iteration i + 1."""
    x = np.array(x0, dtype=np.float64)
    r, p, ap = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    r[free] = (b - apply(x))[free]
    z = precond(r)
    p[free] = z[free]
    prsold = float(r[free] @ z[free])
    res_start = math.sqrt(float(r[free] @ r[free]))
    iterates = []
    if res_start < abs_tol:
        return x, 0, iterates
    for i in range(max_iter):
        ap[free] = apply(p)[free]
        alpha = prsold / float(p[free] @ ap[free])
        x[free] += alpha * p[free]
        r[free] -= alpha * ap[free]
        sqrsnew = math.sqrt(float(r[free] @ r[free]))
        iterates.append(x.copy())
        if sqrsnew / res_start < rel_tol or sqrsnew < abs_tol:
            break
        z = precond(r)
        prsnew = float(r[free] @ z[free])
        p[free] = z[free] + (prsnew / prsold) * p[free]
        prsold = prsnew
    return x, len(iterates), iterates


def identity_preconditioner(r):
    return r.copy()


def sweep_preconditioner(glob, relax=1.0):
    """one forward and one backward sweep of the reference's schedule on a zero start: B r"""
    def precond(r):
        z = glob.sweep(np.zeros(glob.ndof), r, relax, False)
        return glob.sweep(z, r, relax, True)

    return precond


def free_points(glob):
    return ~np.array(glob.boundary, dtype=bool)


def dense_matrix(glob):
    K = np.zeros((glob.ndof, glob.ndof))
    for i, row in enumerate(glob.rows):
        for j, w in row.items():
            K[i, j] = w
    return K


def asymmetry(glob, seed=1, relax=1.0):
    """|<Bu,v> - <u,Bv>| / (|Bu| |v|) of the sweep preconditioner B for two random vectors on the free points"""
    rng = np.random.default_rng(seed)
    free = free_points(glob)
    u, v = np.zeros(glob.ndof), np.zeros(glob.ndof)
    u[free], v[free] = rng.standard_normal(int(free.sum())), rng.standard_normal(int(free.sum()))
    B = sweep_preconditioner(glob, relax)
    Bu, Bv = B(u), B(v)
    return abs(float(Bu[free] @ v[free]) - float(u[free] @ Bv[free])) / (np.linalg.norm(Bu[free]) * np.linalg.norm(v[free]))
