"""Test helper: the multigrid cycle of GeometricMultigridSolver (hyteg_amd/host/solvers.hpp, solveRecursively;
src/hyteg/solvers/GeometricMultigridSolver.hpp:200-305) and the loop of MinResSolver (hyteg_amd/host/minres.hpp;
src/hyteg/solvers/MinresSolver.hpp:88-250) restated in numpy on GLOBAL vectors and matrices, independent of the cell-centric
decomposition and of the host library's exchange plans.

Numbering, matrix and Gauss-Seidel schedule of a level come from hostutil.GlobalSweepOracle (one instance per level, owned by this
module); the prolongation P(l -> l + 1) is built from the geometry of the refinement alone and restriction is its transpose.  The
coarsest level is solved directly.  Everything runs in the dtype of the vectors it is given, so the same code measures its own
rounding: CASE BY CASE, the three cycles (the MINRES iterations) are run in float64 and in numpy.longdouble (80-bit), d is the
largest relative L2 difference of the iterates, and the GPU comparison is bounded by 1e-12 + 50 d (tolerance()).  Nothing is
calibrated against a GPU result.

Measured d (x: the iterates after each of the three cycles; b: the free entries of the restricted right-hand sides the FIRST
cycle leaves on the lower levels, see run_case), largest per group:
    tet_1el 2-4 / 2-5, all smoothers          x 3.3e-16   b 1.2e-14
    regular_octahedron_8el 0-3                x 2.7e-16   b 2.8e-13
    cube_6el 1-3                              x 2.5e-16   b 4.4e-15
    cube_24el outflow 2-3                     x 2.7e-16   b 5.0e-16
    divkgrad, cube_6el 1-3 and tet_1el 2-4    x 1.7e-16   b 6.1e-16
    MINRES, k <= 8, m = 0, 2                  x 5.6e-16
(test_gmg_reference.py prints every value and asserts each <= 1e-12, so no bound exceeds 5.1e-11.)"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import bcutil
import chebyshevutil
import divkgradutil as dk
import hostutil as hu
from oracle import p1_oracle as po

LD = np.longdouble
# the seven edge directions of the 15-point stencil; their parities ( d mod 2 ) are pairwise different
EDGE_DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, -1, 0), (1, 0, -1), (0, 1, -1), (1, -1, 1)]
_BY_PARITY = {tuple(v % 2 for v in d): np.array(d) for d in EDGE_DIRECTIONS}
assert len(_BY_PARITY) == 7


def rel(a, b):
    """relative L2 difference, evaluated in the wider of the two dtypes"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(float(np.sqrt((b * b).sum())), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# levels and the prolongation between them
# ---------------------------------------------------------------------------------------------------------------------
class GlobalLevel:
    """one mesh level: glob (numbering, rows, sweep), the sparse matrix A, its diagonal D, the boolean mask `free` of the points
    Inner | NeumannBoundary selects, and the physical coordinates of every global point"""

    def __init__(self, vertices, cells, level, outflow=False, matrix=None):
        self.level, self.glob = level, hu.GlobalSweepOracle(vertices, cells, level)
        g = self.glob
        self.coords = np.zeros((g.ndof, 3))
        for c, cv in enumerate(g.mesh_cells):
            self.coords[g.gidx[c]] = hu.cell_points(g.vertices[cv].reshape(12), level)
        if outflow:  # bcutil's outflow cube: free = Inner | Neumann, decided from the coordinates
            g.boundary = list(bcutil.point_types(self.coords) == 2)  # host.DirichletBoundary; this instance is ours alone
        self.free = ~np.array(g.boundary, dtype=bool)
        if matrix is None:
            i, j, w = zip(*[(i, j, w) for i, row in enumerate(g.rows) for j, w in row.items()])
            matrix = sp.csr_matrix((w, (i, j)), shape=(g.ndof, g.ndof))
        self.A = sp.csr_matrix(matrix)
        self.D = self.A.diagonal()
        self._wide = None

    def matrix(self, dtype):
        if dtype == np.float64:
            return self.A
        if self._wide is None:
            self._wide = self.A.astype(LD)
        return self._wide

    def apply(self, u):
        return self.matrix(u.dtype) @ u

    def to_global(self, arrays):
        return self.glob.to_global(arrays)

    def to_cells(self, u):
        return self.glob.to_cells(u)


def prolongation(coarse: GlobalLevel, fine: GlobalLevel):
    """the global linear prolongation (n_fine x n_coarse), from geometry alone: in a cell's integer coordinates a fine point with
    even coordinates IS the coarse point p / 2; every other fine point is the midpoint of the coarse points ( p -+ d ) / 2, d the
    edge direction with the parity of p.  A row is set once and has to be identical from every cell that contains the point."""
    assert fine.level == coarse.level + 1
    fine_ijk = po.cell_coords(fine.level).astype(int)
    coarse_pos = {tuple(p): k for k, p in enumerate(po.cell_coords(coarse.level).astype(int))}
    rows = {}
    for gf, gc in zip(fine.glob.gidx, coarse.glob.gidx):
        for k, p in enumerate(fine_ijk):
            if not (p % 2).any():
                row = ((int(gc[coarse_pos[tuple(p // 2)]]), 1.0),)
            else:
                d = _BY_PARITY[tuple(p % 2)]
                a, b = coarse_pos[tuple((p - d) // 2)], coarse_pos[tuple((p + d) // 2)]
                row = tuple(sorted(((int(gc[a]), 0.5), (int(gc[b]), 0.5))))
            assert rows.setdefault(int(gf[k]), row) == row, "a shared point is prolongated differently from two of its cells"
    assert len(rows) == fine.glob.ndof
    i, j, w = zip(*[(i, j, w) for i, row in rows.items() for j, w in row])
    return sp.csr_matrix((w, (i, j)), shape=(fine.glob.ndof, coarse.glob.ndof))


class Hierarchy:
    """levels lo..hi of one mesh, the prolongations between them and the direct solve on the coarsest level"""

    def __init__(self, levels, lo, hi):
        self.lo, self.hi, self.levels = lo, hi, levels
        self.P = {l: prolongation(levels[l], levels[l + 1]) for l in range(lo, hi)}
        self._P_wide = {}

    def prolongate(self, u, level):
        """P( level -> level + 1 ) u"""
        return self._transfer(level, u.dtype) @ u

    def restrict(self, r, level):
        """P( level - 1 -> level )^T r"""
        return self._transfer(level - 1, r.dtype).T @ r

    def _transfer(self, level, dtype):
        if dtype == np.float64:
            return self.P[level]
        if level not in self._P_wide:
            self._P_wide[level] = self.P[level].astype(LD)
        return self._P_wide[level]

    def coarse_solve(self, x, b):
        """A x = b on the free points of level lo with the other entries of x as Dirichlet data (the host: CG to 1e-14).  A dense
        float64 solve, refined three times in the working precision"""
        L = self.levels[self.lo]
        f = L.free
        x = x.copy()
        x[f] = 0
        rhs = (b - L.apply(x))[f]
        Aff = L.A[f][:, f].toarray()
        Aw = Aff.astype(x.dtype)
        y = np.linalg.solve(Aff, rhs.astype(np.float64)).astype(x.dtype)
        for _ in range(3):
            y = y + np.linalg.solve(Aff, (rhs - Aw @ y).astype(np.float64)).astype(x.dtype)
        x[f] = y
        return x


@functools.lru_cache(maxsize=None)
def mesh(name):
    return hu.read_msh(hu.MESHES / f"{name}.msh")


@functools.lru_cache(maxsize=None)
def global_level(name, level, outflow=False):
    v, c = mesh(name)
    return GlobalLevel(v, c, level, outflow)


@functools.lru_cache(maxsize=None)
def hierarchy(name, lo, hi, outflow=False):
    return Hierarchy({l: global_level(name, l, outflow) for l in range(lo, hi + 1)}, lo, hi)


def coefficient(x, y, z):
    """the coefficient of test_gpu_divkgrad_host.py ( coefficient( 2 ) there ): 1.25 + 0.6 * a seeded smooth field, in [0.47, 2.03]"""
    a = np.random.default_rng(2).uniform(1.0, 4.0, 6)
    return 1.25 + 0.6 * (np.sin(a[0] * x + a[1] * y) * np.cos(a[2] * z + a[3]) + 0.3 * np.cos(a[4] * y - a[5] * x))


@functools.lru_cache(maxsize=None)
def divkgrad_hierarchy(name, lo, hi):
    """the same numbering and prolongation with the matrices of -div( k grad u ): k is evaluated on every level at the level's
    points (what P1ElementwiseDivKGrad reads from its coefficient function there).  levels[l].k: the global coefficient vector"""
    v, c = mesh(name)
    levels = {}
    for l in range(lo, hi + 1):
        base = global_level(name, l)
        k = coefficient(base.coords[:, 0], base.coords[:, 1], base.coords[:, 2])
        G, gidx = dk.dense_global(v, c, base.to_cells(k), l)
        # divkgradutil.global_numbering and GlobalSweepOracle number the same points in the same order
        assert len(gidx) == len(base.glob.gidx) and all(np.array_equal(a, b) for a, b in zip(gidx, base.glob.gidx))
        levels[l] = GlobalLevel(v, c, l, matrix=sp.csr_matrix(G))
        levels[l].k = k
    return Hierarchy(levels, lo, hi)


# ---------------------------------------------------------------------------------------------------------------------
# smoothers: callables ( x, b, level ) -> x on global vectors
# ---------------------------------------------------------------------------------------------------------------------
def jacobi_smoother(h: Hierarchy, relax):
    """WeightedJacobiSmoother: x + relax D^-1 ( b - A x ) on the free points"""
    def smooth(x, b, level):
        L = h.levels[level]
        y = x.copy()
        y[L.free] = (x + relax * ((b - L.apply(x)) / L.D))[L.free]
        return y

    return smooth


def sor_smoother(h: Hierarchy, relax=1.0, symmetric=False):
    """SORSmoother / GaussSeidelSmoother: the reference's sweep; symmetric: forward then backward (pcgutil.sweep_preconditioner)"""
    def smooth(x, b, level):
        g = h.levels[level].glob
        y = g.sweep(x, b, relax, False)
        return g.sweep(y, b, relax, True) if symmetric else y

    return smooth


def chebyshev_smoother(h: Hierarchy, order, radii):
    """ChebyshevSmoother( order ) with the bounds 0.3 rho / 1.2 rho: the recurrence of chebyshevutil.smooth_cell on the global
    operator.  radii: {level: spectral radius of D^-1 A}"""
    coeff = {l: chebyshevutil.coefficients(order, 0.3 * r, 1.2 * r) for l, r in radii.items()}

    def smooth(x, b, level):
        L, c = h.levels[level], coeff[level]
        x = x.copy()
        t1 = np.zeros_like(x)
        t1[L.free] = ((b - L.apply(x)) / L.D)[L.free]
        x[L.free] += c[0] * t1[L.free]
        for k in range(1, len(c)):
            t1[L.free] = (L.apply(t1) / L.D)[L.free]
            x[L.free] += c[k] * t1[L.free]
        return x

    return smooth


def spectral_radius(L: GlobalLevel, iters=100, seed=0):
    """spectral radius of D^-1 A on the free points of a level: `iters` power iterations (chebyshevutil.radius_cell, globally)"""
    v = np.zeros(L.glob.ndof)
    v[L.free] = np.random.default_rng(seed).random(int(L.free.sum()))
    rho = 0.0
    for _ in range(iters):
        v /= np.linalg.norm(v)
        y = np.where(L.free, L.apply(v) / L.D, 0.0)
        rho = float(v @ y)
        v = y
    return rho


# ---------------------------------------------------------------------------------------------------------------------
# the cycle
# ---------------------------------------------------------------------------------------------------------------------
def cycle(h: Hierarchy, smoother, xs, bs, level, pre, post, wcycle=False):
    """solveRecursively statement by statement; xs[l], bs[l]: the global vectors of x and b on level l, updated in place (the
    host's functions carry all levels, and the cycle leaves its restricted residuals in b and its corrections in x there)"""
    if level == h.lo:
        xs[level] = h.coarse_solve(xs[level], bs[level])
        return
    L, C = h.levels[level], h.levels[level - 1]
    for _ in range(pre):
        xs[level] = smoother(xs[level], bs[level], level)
    r = np.zeros_like(xs[level])
    r[L.free] = (bs[level] - L.apply(xs[level]))[L.free]
    bs[level - 1] = bs[level - 1].copy()
    bs[level - 1][C.free] = h.restrict(r, level)[C.free]  # the other points keep their value
    xs[level - 1] = np.zeros_like(xs[level - 1])  # on ALL points
    cycle(h, smoother, xs, bs, level - 1, pre, post, wcycle)
    if wcycle:
        cycle(h, smoother, xs, bs, level - 1, pre, post, wcycle)
    xs[level] = xs[level].copy()
    xs[level][L.free] += h.prolongate(xs[level - 1], level - 1)[L.free]
    for _ in range(post):
        xs[level] = smoother(xs[level], bs[level], level)


# ---------------------------------------------------------------------------------------------------------------------
# MINRES
# ---------------------------------------------------------------------------------------------------------------------
def minres(apply, precond, x0, b, free, max_iter, rel_tol=0.0, abs_tol=1e-16):
    """MinResSolver::solve statement by statement.  apply(u): A u on a global vector; precond(r): z from M z = r, a global vector
    that vanishes outside `free`.  Returns (x, [eta after every iteration])."""
    x = np.array(x0)
    zero = np.zeros_like(x)
    vm, v, vp, z, zp, wm, w, wp = (zero.copy() for _ in range(8))
    v[free] = (b - apply(x))[free]
    z = precond(v)
    gamma_old, gamma_new = 1.0, np.sqrt(z[free] @ v[free])
    res_start = gamma_new
    eta, s_old, s_new, c_old, c_new = gamma_new, 0.0, 0.0, 1.0, 1.0
    etas = []
    if gamma_new < abs_tol:
        return x, etas
    for _ in range(max_iter):
        z[free] = (1.0 / gamma_new) * z[free]
        vp[free] = apply(z)[free]
        delta = vp[free] @ z[free]
        vp[free] = vp[free] - (delta / gamma_new) * v[free] - (gamma_new / gamma_old) * vm[free]
        zp = precond(vp)
        gamma_old, gamma_new = gamma_new, np.sqrt(zp[free] @ vp[free])
        alpha0 = c_new * delta - c_old * s_new * gamma_old
        alpha1 = np.sqrt(alpha0 * alpha0 + gamma_new * gamma_new)
        alpha2 = s_new * delta + c_old * c_new * gamma_old
        alpha3 = s_old * gamma_old
        c_old, c_new = c_new, alpha0 / alpha1
        s_old, s_new = s_new, gamma_new / alpha1
        wp[free] = (1.0 / alpha1) * z[free] - (alpha3 / alpha1) * wm[free] - (alpha2 / alpha1) * w[free]
        x[free] += (c_new * eta) * wp[free]
        eta = -s_new * eta
        vm, v, vp = v, vp, vm
        wm, w, wp = w, wp, wm
        z, zp = zp, z
        etas.append(eta)
        if abs(eta) / res_start < rel_tol or abs(eta) < abs_tol or not np.isfinite(float(eta)):
            break
    return x, etas


def identity_preconditioner(free):
    return lambda r: np.where(free, r, 0)


def jacobi_preconditioner(L: GlobalLevel, iterations):
    """JacobiPreconditioner::solve: x = b, then `iterations` Jacobi steps with relax 1, on the free points"""
    def precond(r):
        x = np.where(L.free, r, 0)
        for _ in range(iterations):
            x = np.where(L.free, x + (r - L.apply(x)) / L.D, 0)
        return x

    return precond


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test files run, their inputs, the restated results and the measured tolerance
# ---------------------------------------------------------------------------------------------------------------------
# smoother: "jacobi" (relax), "gs", "sor" (relax), "sgs", "ssor" (relax), "chebyshev" (order)
GmgCase = namedtuple("GmgCase", "mesh lo hi smoother relax order pre post wcycle outflow divkgrad",
                     defaults=(1.0, 0, 1, 1, False, False, False))
CYCLES = 3


def _tet_cases():
    kinds = [("jacobi", 2.0 / 3.0, 0), ("gs", 1.0, 0), ("sor", 1.3, 0), ("sgs", 1.0, 0), ("chebyshev", 1.0, 3)]
    out = [GmgCase("tet_1el", 2, 4, s, r, o, pre, post) for s, r, o in kinds for pre, post in ((3, 3), (1, 2))]
    return out + [GmgCase("tet_1el", 2, 5, "gs", 1.0, 0, 1, 1, True)]


def _multi_cell_cases():
    kinds = [("jacobi", 2.0 / 3.0, 0), ("gs", 1.0, 0), ("ssor", 1.3, 0), ("chebyshev", 1.0, 2)]
    return [GmgCase(m, lo, hi, s, r, o, pre, post, w) for m, lo, hi in (("regular_octahedron_8el", 0, 3), ("cube_6el", 1, 3))
            for s, r, o in kinds for pre, post, w in ((2, 2, False), (1, 1, True))]


TET_CASES = _tet_cases()
MULTI_CELL_CASES = _multi_cell_cases()
OUTFLOW_CASES = [GmgCase("cube_24el", 2, 3, s, r, 0, 2, 2, False, True) for s, r in (("jacobi", 2.0 / 3.0), ("gs", 1.0))]
DIVKGRAD_CASES = [GmgCase(m, lo, hi, s, 2.0 / 3.0, o, pre, post, False, False, True)
                  for m, lo, hi in (("cube_6el", 1, 3), ("tet_1el", 2, 4)) for s, o, pre, post in (("jacobi", 0, 2, 2), ("chebyshev", 2, 1, 1))]
GMG_CASES = TET_CASES + MULTI_CELL_CASES + OUTFLOW_CASES + DIVKGRAD_CASES


def case_id(c):
    name = {"jacobi": f"jacobi{c.relax:.2f}", "sor": f"sor{c.relax}", "ssor": f"ssor{c.relax}", "chebyshev": f"chebyshev{c.order}"}.get(c.smoother, c.smoother)
    return f"{'divkgrad-' if c.divkgrad else ''}{c.mesh}{'-outflow' if c.outflow else ''}-{c.lo}-{c.hi}-{name}-{'W' if c.wcycle else 'V'}{c.pre}{c.post}"


def case_hierarchy(c):
    return divkgrad_hierarchy(c.mesh, c.lo, c.hi) if c.divkgrad else hierarchy(c.mesh, c.lo, c.hi, c.outflow)


@functools.lru_cache(maxsize=None)
def case_radii(c):
    """{level: radius} for the Chebyshev cases (every level lo..hi: the host wants one per level).  One macro-cell with the constant
    operator: chebyshevutil.radius_cell (level 2 has ONE inner point: D^-1 A = 1 there); otherwise the global power iteration"""
    h = case_hierarchy(c)
    if c.mesh == "tet_1el" and not c.divkgrad:
        co = h.levels[c.lo].glob.vertices[h.levels[c.lo].glob.mesh_cells[0]].reshape(12)
        return {l: chebyshevutil.radius_cell(l, po.assemble_cell_stencil(co, l), iters=100) for l in range(c.lo, c.hi + 1)}
    return {l: spectral_radius(h.levels[l]) for l in range(c.lo, c.hi + 1)}


def case_smoother(c):
    h = case_hierarchy(c)
    if c.smoother == "jacobi":
        return jacobi_smoother(h, c.relax)
    if c.smoother in ("gs", "sor"):
        return sor_smoother(h, c.relax)
    if c.smoother in ("sgs", "ssor"):
        return sor_smoother(h, c.relax, symmetric=True)
    assert c.smoother == "chebyshev"
    return chebyshev_smoother(h, c.order, case_radii(c))


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """(xs, bs): per level the global start vectors.  Top level: x random (not smooth; one value per global point, so every copy of
    a shared point agrees) and zero on the Dirichlet points, b random on the free points.  Lower levels: junk on ALL points of x
    and b -- a cycle that zeroes the coarse iterate on the free points only, or writes b outside them, is then seen"""
    h = case_hierarchy(c)
    rng = np.random.default_rng(100 + GMG_CASES.index(c))
    xs, bs = {}, {}
    for l in range(c.hi, c.lo - 1, -1):
        n, free = h.levels[l].glob.ndof, h.levels[l].free
        xs[l], bs[l] = rng.standard_normal(n), rng.standard_normal(n)
        if l == c.hi:
            xs[l], bs[l] = np.where(free, xs[l], 0.0), np.where(free, bs[l], 0.0)
        for a in (xs[l], bs[l]):
            a.setflags(write=False)
    return xs, bs


def run_case(c, dtype=np.float64):
    """CYCLES cycles: ([x on the top level after every cycle], {level: b below the top after the FIRST cycle},
    {level: x below the top after the last cycle}).  b is taken after the first cycle because the restricted residuals of later
    cycles are ill-conditioned data: b - A x cancels more digits the further the iteration has converged (80-bit against float64
    after the third cycle: up to 3e-12 with the fast smoothers), while a wrong flag or level shows in the first cycle already"""
    h, smoother = case_hierarchy(c), case_smoother(c)
    xs0, bs0 = case_inputs(c)
    xs, bs = {l: a.astype(dtype) for l, a in xs0.items()}, {l: a.astype(dtype) for l, a in bs0.items()}
    iterates, b_lower = [], None
    for _ in range(CYCLES):
        cycle(h, smoother, xs, bs, c.hi, c.pre, c.post, c.wcycle)
        iterates.append(xs[c.hi].copy())
        if b_lower is None:
            b_lower = {l: bs[l].copy() for l in range(c.lo, c.hi)}
    return iterates, b_lower, {l: xs[l] for l in range(c.lo, c.hi)}


Restated = namedtuple("Restated", "iterates b_lower x_lower d_x d_b")


@functools.lru_cache(maxsize=None)
def restated(c):
    """the float64 results of run_case with the measured rounding: d_x (d_b) = the largest relative L2 difference between the
    float64 and the 80-bit run over the iterates (over the free entries of the lower levels' b after the first cycle)"""
    it, b, x = run_case(c)
    it_w, b_w, _ = run_case(c, LD)
    free = {l: case_hierarchy(c).levels[l].free for l in b}  # the other entries of b are the junk of case_inputs, of another size
    return Restated(it, b, x, max(rel(a, w) for a, w in zip(it, it_w)), max(rel(b[l][free[l]], b_w[l][free[l]]) for l in b))


def tolerance(d):
    """the bound of a GPU comparison whose restatement differs by d between float64 and 80-bit arithmetic: the project's parity bar
    for one kernel plus 50 d for a different but equally valid summation order in every kernel of the chain"""
    return 1e-12 + 50.0 * d


MinresCase = namedtuple("MinresCase", "mesh level outflow k m")
MINRES_CASES = [MinresCase(mesh_, 2, outflow, k, m) for mesh_, outflow in (("regular_octahedron_8el", False), ("cube_24el", True))
                for m in (0, 2) for k in (1, 2, 3, 5, 8)]


def minres_id(c):
    return f"{c.mesh}{'-outflow' if c.outflow else ''}-{c.level}-k{c.k}-jacobi{c.m}"


@functools.lru_cache(maxsize=None)
def minres_inputs(mesh_, level, outflow):
    """(x0, b): nonzero Dirichlet data, a random start on the free points, zero right-hand side"""
    L = global_level(mesh_, level, outflow)
    x0 = np.random.default_rng(7).standard_normal(L.glob.ndof)
    x0.setflags(write=False)
    return x0, np.zeros(L.glob.ndof)


def run_minres(c, dtype=np.float64, rel_tol=0.0):
    L = global_level(c.mesh, c.level, c.outflow)
    x0, b = minres_inputs(c.mesh, c.level, c.outflow)
    precond = jacobi_preconditioner(L, c.m) if c.m > 0 else identity_preconditioner(L.free)
    return minres(L.apply, precond, x0.astype(dtype), b.astype(dtype), L.free, c.k, rel_tol)


MinresRestated = namedtuple("MinresRestated", "x etas d_x")


@functools.lru_cache(maxsize=None)
def minres_restated(c):
    x, etas = run_minres(c)
    x_w, _ = run_minres(c, LD)
    return MinresRestated(x, etas, rel(x, x_w))
