"""Helpers of the tests of the fused residual and Chebyshev kernel modes of the variable-coefficient P1 operators: the arithmetic
of each mode restated in numpy on top of an ( A src ) of epsilonutil.apply_cell / divkgradutil.apply_cell, a smooth coefficient, and
one calling convention for both operators (arrays of shape ( NC, n ); NC = 3 for epsilon, 1 for div-k-grad).  Below that, the multigrid cycle
on the epsilon operator and the block-preconditioned MINRES restated on global matrices, with the cases the CPU and the GPU tests
share.  Nothing here calls the library under test except the Operator adapters, which only forward to hyteg_amd.capi."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import divkgradutil as du
import epsilonutil as eu
import gmgutil as gm


def smooth_coefficient(tet, level, contrast=20.0):
    """0.5 * contrast^s, s in [0, 1] linear in the physical coordinates: smooth, max / min = contrast over the cell's points"""
    X = du.cell_points(tet, level)
    s = X @ np.array([1.3, -0.7, 0.9])
    s = (s - s.min()) / (s.max() - s.min())
    return 0.5 * contrast**s


# ---- the arithmetic of the modes, with the association the kernels are written in ----
def residual(A_src, rhs):
    return rhs - A_src


def chebyshev_start(A_x, rhs, inv_diag):
    return inv_diag * (rhs - A_x)


def chebyshev_step(A_tin, t_in, x, inv_diag, c_prev, c_cur, has_prev):
    """(t_out, x_new)"""
    t_out = inv_diag * A_tin
    return t_out, ((x + c_prev * t_in) if has_prev else x) + c_cur * t_out


class Operator:
    """one calling convention for the C-ABI entries of both operators; every array argument is a list of NC device pointers"""

    def __init__(self, capi, name):
        self.capi, self.name = capi, name
        self.nc = 3 if name == "epsilon" else 1
        self.shapes = capi.EPSILON_SHAPES if name == "epsilon" else capi.DIVKGRAD_SHAPES

    def _f(self, what):
        return getattr(self.capi, f"p1_elementwise_{self.name}_{what}")

    def _a(self, ptrs):
        return ptrs if self.nc == 3 else ptrs[0]

    def _kw(self, comps):
        return {} if self.nc == 1 else {"comps": (1 << self.nc) - 1 if comps is None else comps}

    def apply_reference(self, src, coef, tet, level):
        if self.nc == 3:
            return eu.apply_cell(src, coef, tet, level)
        return du.apply_cell(src[0], coef, tet, level)[None, :]

    def residual(self, dst, src, rhs, coef, tet, level, comps=None):
        self._f("residual_macro_3d")(self._a(dst), self._a(src), self._a(rhs), coef, tet, 1 << level, **self._kw(comps))

    def chebyshev_start(self, t_out, rhs, x, inv_diag, coef, tet, level, comps=None):
        self._f("chebyshev_start_macro_3d")(self._a(t_out), self._a(rhs), self._a(x), self._a(inv_diag), coef, tet, 1 << level, **self._kw(comps))

    def chebyshev_step(self, t_out, x, t_in, inv_diag, coef, tet, level, c_prev, c_cur, has_prev, comps=None):
        self._f("chebyshev_step_macro_3d")(self._a(t_out), self._a(x), self._a(t_in), self._a(inv_diag), coef, tet, 1 << level, c_prev, c_cur,
                                           has_prev, **self._kw(comps))

    def set_shape(self, ny=0, lz=0):
        self._f("set_shape")(ny, lz)

    def set_inner_by_points(self, on):
        self._f("set_inner_by_points")(on)


# ---------------------------------------------------------------------------------------------------------------------
# The multigrid cycle on the epsilon operator and the block-preconditioned MINRES, restated on global matrices with what
# tests/gmgutil.py has: its Hierarchy with the prolongation I_3 (x) P (component-major vectors: u entries, v entries, w entries), its
# cycle, smoothers and MINRES loop.  Velocity under the storage's default condition (Dirichlet on the mesh boundary).
# ---------------------------------------------------------------------------------------------------------------------
def contrast40(x, y, z):
    """the viscosity of tests/test_gpu_epsilon_host.py: exp( 3 x ) ( 1 + y ), contrast 40 on the unit cube"""
    return np.exp(3.0 * x) * (1.0 + y)


def unit_viscosity(x, y, z):
    return np.ones_like(x)


VISCOSITIES = {"contrast40": contrast40, "one": unit_viscosity}


class VectorLevel:
    """what gmgutil's cycle, smoothers and coarse solve read of a level, for three components over the scalar level `base`"""

    def __init__(self, base, matrix, mu):
        self.level, self.base, self.mu = base.level, base, mu
        self.n = base.glob.ndof
        self.A = sp.csr_matrix(matrix)
        self.D = self.A.diagonal()
        self.free = np.tile(base.free, 3)
        self._wide = None

    def matrix(self, dtype):
        if dtype == np.float64:
            return self.A
        if self._wide is None:
            self._wide = self.A.astype(gm.LD)
        return self._wide

    def apply(self, u):
        return self.matrix(u.dtype) @ u


class VectorHierarchy(gm.Hierarchy):
    """gmgutil.Hierarchy with the scalar prolongation on every component"""

    def __init__(self, levels, scalar):
        self.lo, self.hi, self.levels, self.scalar = scalar.lo, scalar.hi, levels, scalar
        self.P = {l: sp.kron(sp.identity(3), scalar.P[l], format="csr") for l in scalar.P}
        self._P_wide = {}


@functools.lru_cache(maxsize=None)
def epsilon_hierarchy(name, lo, hi, viscosity="contrast40"):
    v, c = gm.mesh(name)
    scalar = gm.hierarchy(name, lo, hi)
    levels = {}
    for l in range(lo, hi + 1):
        base = scalar.levels[l]
        mu = VISCOSITIES[viscosity](base.coords[:, 0], base.coords[:, 1], base.coords[:, 2])
        A, gidx, n = eu.dense_global(v, c, base.to_cells(mu), l)
        # epsilonutil's numbering and GlobalSweepOracle's number the same points in the same order
        assert n == base.glob.ndof and all(np.array_equal(a, b) for a, b in zip(gidx, base.glob.gidx))
        levels[l] = VectorLevel(base, A, mu)
    return VectorHierarchy(levels, scalar)


def radii(h):
    """{level: spectral radius of D^-1 A on the free points}: gmgutil.spectral_radius works on anything with free, apply, D"""
    out = {}
    for l, L in h.levels.items():
        v = np.zeros(3 * L.n)
        v[L.free] = np.random.default_rng(0).random(int(L.free.sum()))
        rho = 0.0
        for _ in range(100):
            v /= np.linalg.norm(v)
            y = np.where(L.free, L.apply(v) / L.D, 0.0)
            rho, v = float(v @ y), y
        out[l] = rho
    return out


def smoother(h, kind, order_or_relax, rho=None):
    if kind == "jacobi":
        return gm.jacobi_smoother(h, order_or_relax)
    assert kind == "chebyshev"
    return gm.chebyshev_smoother(h, order_or_relax, rho if rho is not None else radii(h))


def cycles(h, smooth, x_top, b_top, pre, post, n, dtype=np.float64):
    """n V-cycles on the top level from x_top: the iterates.  The lower levels start from zero (the cycle overwrites them)"""
    xs = {l: np.zeros(3 * h.levels[l].n, dtype=dtype) for l in range(h.lo, h.hi + 1)}
    bs = {l: np.zeros(3 * h.levels[l].n, dtype=dtype) for l in range(h.lo, h.hi + 1)}
    xs[h.hi], bs[h.hi] = x_top.astype(dtype), b_top.astype(dtype)
    out = []
    for _ in range(n):
        gm.cycle(h, smooth, xs, bs, h.hi, pre, post)
        out.append(xs[h.hi].copy())
    return out


def cycle_action(h, smooth, pre, post, velocity_cycles=1):
    """r -> the iterate after velocity_cycles V-cycles on A z = r from z = 0 (zero outside the free points): the velocity action of
    the block preconditioner"""
    def action(r):
        r = np.where(h.levels[h.hi].free, r, 0)
        return cycles(h, smooth, np.zeros_like(r), r, pre, post, velocity_cycles, r.dtype)[-1]

    return action


def block_preconditioner(h, smooth, pre, post, pressure_scale, velocity_cycles=1):
    """the action of StokesVectorBlockDiagonalPreconditioner on a global Stokes vector ( u, v, w, p ): the cycle on the velocity, the
    pointwise scaling pressure_scale on the pressure"""
    velocity = cycle_action(h, smooth, pre, post, velocity_cycles)
    n3 = 3 * h.levels[h.hi].n

    def precond(r):
        return np.concatenate([velocity(r[:n3]), pressure_scale.astype(r.dtype) * r[n3:]])

    return precond


# ---------------------------------------------------------------------------------------------------------------------
# the cases the CPU test pins and the GPU tests compare with: inputs, restated results, measured rounding d (float64 against 80-bit)
# ---------------------------------------------------------------------------------------------------------------------
CycleCase = namedtuple("CycleCase", "mesh lo hi smoother param pre post")
CYCLE_CASES = [CycleCase(m, lo, hi, s, p, pre, post) for m, lo, hi in (("cube_6el", 1, 3), ("tet_1el", 2, 4))
               for s, p, pre, post in (("chebyshev", 2, 1, 1), ("jacobi", 2.0 / 3.0, 2, 2))]
CYCLES = 3


def cycle_id(c):
    return f"{c.mesh}-{c.lo}-{c.hi}-{c.smoother}{c.param:.3g}-V{c.pre}{c.post}"


@functools.lru_cache(maxsize=None)
def case_radii(mesh, lo, hi, viscosity="contrast40"):
    return radii(epsilon_hierarchy(mesh, lo, hi, viscosity))


@functools.lru_cache(maxsize=None)
def top_inputs(mesh, lo, hi, seed=0):
    """(x0, b) on the top level: random on the free points, zero on the fixed ones"""
    L = epsilon_hierarchy(mesh, lo, hi).levels[hi]
    rng = np.random.default_rng(4000 + seed)
    x0, b = (np.where(L.free, rng.standard_normal(3 * L.n), 0.0) for _ in range(2))
    x0.setflags(write=False), b.setflags(write=False)
    return x0, b


def run_cycles(c, dtype=np.float64):
    """(iterates after each of CYCLES cycles, residual reduction of each cycle)"""
    h = epsilon_hierarchy(c.mesh, c.lo, c.hi)
    smooth = smoother(h, c.smoother, c.param, case_radii(c.mesh, c.lo, c.hi))
    x0, b = top_inputs(c.mesh, c.lo, c.hi)
    its = cycles(h, smooth, x0, b, c.pre, c.post, CYCLES, dtype)
    L = h.levels[c.hi]
    res = [np.linalg.norm(np.where(L.free, b.astype(dtype) - L.apply(x), 0).astype(np.float64)) for x in [x0.astype(dtype)] + its]
    return its, [res[k + 1] / res[k] for k in range(CYCLES)]


RestatedCycles = namedtuple("RestatedCycles", "iterates rates d d_rate")


@functools.lru_cache(maxsize=None)
def restated_cycles(c):
    it, rates = run_cycles(c)
    it_w, rates_w = run_cycles(c, gm.LD)
    return RestatedCycles(it, rates, max(gm.rel(a, w) for a, w in zip(it, it_w)), max(abs(a - w) / w for a, w in zip(rates, rates_w)))


def smoother_call(mesh, lo, hi, order, dtype=np.float64, free=None):
    """(residual b - A x on the free points, x after ONE Chebyshev( order ) call) on the top level from top_inputs; free: another
    selection of the top level's points than the default condition's"""
    h = epsilon_hierarchy(mesh, lo, hi)
    L = h.levels[hi]
    x0, b = top_inputs(mesh, lo, hi, 1)
    if free is not None:  # junk becomes data on the points that are free now
        rng = np.random.default_rng(4100)
        x0, b = (np.where(free, rng.standard_normal(3 * L.n), 0.0) for _ in range(2))
        keep, L.free = L.free, free
    try:
        x0, b = x0.astype(dtype), b.astype(dtype)
        r = np.where(L.free, b - L.apply(x0), 0)
        x = gm.chebyshev_smoother(h, order, case_radii(mesh, lo, hi))(x0, b, hi)
    finally:
        if free is not None:
            L.free = keep
    return x0, b, r, x


# ---- block-preconditioned MINRES on cube_6el, level 2 (velocity hierarchy 1..2), contrast-40 viscosity ----
MINRES_MESH, MINRES_LO, MINRES_LEVEL = "cube_6el", 1, 2
MINRES_KS = (1, 3, 8)


@functools.lru_cache(maxsize=None)
def minres_problem():
    """the dense Stokes matrix, the free DoFs ( velocity: the default condition; pressure: all ), a random exact solution with
    mean-free pressure, b = S exact, a start that carries the exact Dirichlet values, and the lumped mass"""
    h = epsilon_hierarchy(MINRES_MESH, MINRES_LO, MINRES_LEVEL)
    L = h.levels[MINRES_LEVEL]
    v, c = gm.mesh(MINRES_MESH)
    S, gidx, n = eu.dense_stokes_global(v, c, L.base.to_cells(L.mu), MINRES_LEVEL)
    free = np.concatenate([L.free, np.ones(n, dtype=bool)])
    rng = np.random.default_rng(4200)
    exact = rng.uniform(-1.0, 1.0, 4 * n)
    exact[3 * n:] -= exact[3 * n:].mean()
    b = S @ exact
    start = np.where(free, rng.uniform(-1.0, 1.0, 4 * n), exact)
    lumped = eu.lumped_mass_global(v, c, MINRES_LEVEL, gidx, n)
    for a in (S, free, exact, b, start, lumped):
        a.setflags(write=False)
    return S, free, exact, b, start, lumped, n


def minres_preconditioner(kind, order=2, pre=1, post=1):
    """the restated "block" / "block_viscosity" preconditioner with the Chebyshev( order ) V( pre, post ) cycle"""
    h = epsilon_hierarchy(MINRES_MESH, MINRES_LO, MINRES_LEVEL)
    S, free, exact, b, start, lumped, n = minres_problem()
    scale = (h.levels[MINRES_LEVEL].mu if kind == "block_viscosity" else 1.0) / lumped
    smooth = smoother(h, "chebyshev", order, case_radii(MINRES_MESH, MINRES_LO, MINRES_LEVEL))
    return block_preconditioner(h, smooth, pre, post, scale)


def run_minres(kind, k, dtype=np.float64, rel_tol=0.0):
    S, free, exact, b, start, lumped, n = minres_problem()
    Sw = S.astype(dtype)
    return gm.minres(lambda u: Sw @ u, minres_preconditioner(kind), start.astype(dtype), b.astype(dtype), free, k, rel_tol)


@functools.lru_cache(maxsize=None)
def restated_minres(kind, k):
    """(x after k iterations, d)"""
    x, _ = run_minres(kind, k)
    x_w, _ = run_minres(kind, k, gm.LD)
    return x, gm.rel(x, x_w)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side: global vectors <-> the functions of the host layer (hyteg_amd.host, tests/hostutil.py are handed in by the tests)
# ---------------------------------------------------------------------------------------------------------------------
class Device:
    """a storage of one mesh with the maps between global vectors of a level and the cell arrays of its functions"""

    def __init__(self, host, hu, stream, mesh, lo, hi, viscosity="contrast40"):
        self.host, self.hu, self.mesh, self.lo, self.hi = host, hu, mesh, lo, hi
        self.h = epsilon_hierarchy(mesh, lo, hi, viscosity)
        self.st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
        self.st.set_stream(stream)
        self.owned = []
        self.mu = self.scalar("mu", {l: self.h.levels[l].mu for l in range(lo, hi + 1)})

    def idx(self, level):
        gidx = self.h.levels[level].base.glob.gidx
        return [gidx[self.st.local_cell(i)[0]] for i in range(self.st.n_local_cells)]

    def scalar(self, name, by_level):
        """a P1Function on levels lo..hi holding the global vectors by_level[l]"""
        f = self.host.P1Function(self.st, name, self.lo, self.hi)
        for l, vec in by_level.items():
            self.hu.upload(f, eu.to_cells(np.asarray(vec, dtype=np.float64), self.idx(l)), l)
        self.owned.append(f)
        return f

    def vector(self, name, top):
        """three P1Functions on levels lo..hi; the top level holds the component-major global vector `top`"""
        n = self.h.levels[self.hi].n
        return [self.scalar(f"{name}{k}", {self.hi: top[k * n:(k + 1) * n]}) for k in range(3)]

    def read(self, fs, level=None):
        """the component-major global vector of three functions"""
        level = self.hi if level is None else level
        n = self.h.levels[level].n
        return np.concatenate([eu.to_global(self.hu.download(f, level), self.idx(level), n) for f in fs])

    def operator(self):
        op = self.host.P1ElementwiseAffineEpsilonOperator(self.st, self.lo, self.hi, self.mu)
        op.compute_inverse_diagonal()
        self.owned.append(op)
        return op

    def radii(self):
        r = case_radii(self.mesh, self.lo, self.hi)
        return [r[l] for l in range(self.lo, self.hi + 1)]

    def close(self):
        for o in reversed(self.owned):
            o.close()
        self.st.close()
