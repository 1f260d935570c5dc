"""The multigrid cycle on the P2 epsilon operator and the block-preconditioned MINRES of the Taylor-Hood system, restated on global
matrices: p2epsilonutil.global_matrix per level, p2divkgradutil.prolongation on every component (component-major vectors: u entries, v
entries, w entries), and the cycle, smoothers, mode arithmetic and MINRES loop of gmgutil / epsilongmgutil.  Velocity under the storage's
default condition: Dirichlet on the boundary of the unit cube."""
import functools

import numpy as np
import scipy.sparse as sp

import epsilongmgutil as eg
import gmgutil as gm
import p2divkgradutil as pu
import p2epsilonutil as pe


class Level:
    """what gmgutil's cycle, smoothers and coarse solve and epsilongmgutil's cycles read of a level"""

    def __init__(self, level, A, gidx, n, free_scalar, mus):
        self.level, self.n, self.gidx, self.mus = level, n, gidx, mus
        self.A = sp.csr_matrix(A)
        self.D = self.A.diagonal()
        self.free = np.tile(free_scalar, 3)
        self._wide = None

    def matrix(self, dtype):
        if dtype == np.float64:
            return self.A
        if self._wide is None:
            self._wide = self.A.astype(gm.LD)
        return self._wide

    def apply(self, u):
        return self.matrix(u.dtype) @ u


class Hierarchy(gm.Hierarchy):
    """gmgutil.Hierarchy over P2 levels: the quadratic prolongation on every component, restriction its transpose"""

    def __init__(self, levels, lo, hi):
        self.lo, self.hi, self.levels = lo, hi, levels
        self.P = {}
        for l in range(lo, hi):
            C, F = levels[l], levels[l + 1]
            self.P[l] = sp.kron(sp.identity(3), pu.prolongation(l, C.gidx, C.n, F.gidx, F.n), format="csr")
        self._P_wide = {}


def lowest_level(name):
    """the lowest level at which the mesh has a free velocity DoF"""
    v, c = gm.mesh(name)
    for l in range(0, 4):
        gidx, n = pu.global_numbering(c, l)
        if not pe.boundary_dofs(v, c, l, gidx, n).all():
            return l
    raise AssertionError("no free DoF up to level 3")


@functools.lru_cache(maxsize=None)
def hierarchy(name, lo, hi, viscosity="contrast40"):
    v, c = (np.asarray(a) for a in gm.mesh(name))
    levels = {}
    for l in range(lo, hi + 1):
        mus = [eg.VISCOSITIES[viscosity](*pu.dof_points(np.asarray(v, dtype=np.float64)[cv], l).T) for cv in c]
        A, gidx, n = pe.global_matrix(v, c, mus, l)
        levels[l] = Level(l, A, gidx, n, ~pe.boundary_dofs(v, c, l, gidx, n), mus)
    return Hierarchy(levels, lo, hi)


@functools.lru_cache(maxsize=None)
def stokes_problem(name, lo, hi, viscosity="contrast40", seed=1400):
    """the Taylor-Hood system on the top level with a random exact solution (mean-free pressure), b = S exact, a random start; the free
    mask, the lumped pressure mass and the viscosity at the pressure DoFs.  Read-only"""
    h = hierarchy(name, lo, hi, viscosity)
    v, c = (np.asarray(a) for a in gm.mesh(name))
    top = h.levels[hi]
    S, gidx, n, pidx, npr = pe.taylor_hood_matrix(v, c, top.mus, hi)
    rng = np.random.default_rng(seed)
    exact = rng.uniform(-1.0, 1.0, 3 * n + npr)
    exact[3 * n:] -= exact[3 * n:].mean()
    x0 = rng.uniform(-1.0, 1.0, 3 * n + npr)
    free = np.concatenate([top.free, np.ones(npr, dtype=bool)])
    lumped = pe.lumped_pressure_mass(v, c, hi, pidx, npr)
    mu_p, nv = np.zeros(npr), pu.vertex_size(hi)
    for ix, mu_c in zip(pidx, top.mus):
        mu_p[ix] = mu_c[:nv]
    out = dict(S=S.toarray(), b=S @ exact, exact=exact, start=np.where(free, x0, exact), free=free, lumped=lumped, mu_p=mu_p, pidx=pidx, npr=npr)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def minres(name, lo, hi, kind, max_iter, rel_tol=0.0, dtype=np.float64, order=2, pre=1, post=1):
    """the restated MINRES loop with preconditioner "pressure", "pressure_viscosity", "block" or "block_viscosity" (V( pre, post )
    Chebyshev( order ) cycle on the velocity); returns what gmgutil.minres returns"""
    p, h = stokes_problem(name, lo, hi), hierarchy(name, lo, hi)
    free = p["free"]
    n3 = len(free) - p["npr"]
    scale_p = ((p["mu_p"] if kind.endswith("viscosity") else 1.0) / p["lumped"]).astype(dtype)
    if kind.startswith("block"):
        inner = eg.block_preconditioner(h, eg.smoother(h, "chebyshev", order), pre, post, scale_p)
        precond = lambda r: np.where(free, inner(r), 0)  # noqa: E731
    else:
        scale = np.concatenate([np.ones(n3, dtype=dtype), scale_p])
        precond = lambda r: np.where(free, scale * r, 0)  # noqa: E731
    Sw = p["S"].astype(dtype)
    return gm.minres(lambda u: Sw @ u, precond, p["start"].astype(dtype), p["b"].astype(dtype), free, max_iter, rel_tol)


class Device:
    """a host storage with the numberings of a restated hierarchy: P2 functions over the levels lo..hi, filled on the top level from global
    vectors; the viscosity on every level"""

    def __init__(self, host, hu, stream, name, lo, hi):
        self.host, self.hu, self.lo, self.hi = host, hu, lo, hi
        self.h = hierarchy(name, lo, hi)
        self.st = host.Storage.from_gmsh(hu.MESHES / f"{name}.msh")
        self.st.set_stream(stream)
        self.ids = [self.st.local_cell(i)[0] for i in range(self.st.n_local_cells)]
        self.nv = pu.vertex_size(hi)
        self.mu = host.P2Function(self.st, "mu", lo, hi)
        for l in range(lo, hi + 1):
            nv = pu.vertex_size(l)
            for c, i in enumerate(self.ids):
                a = np.ascontiguousarray(self.h.levels[l].mus[i])
                self.mu.upload(l, a[:nv], a[nv:], cell=c)
        self.open = [self.mu]

    def operator(self):
        op = self.host.P2ViscousBlockEpsilonOperator(self.st, self.lo, self.hi, self.mu)
        op.compute_inverse_diagonal()
        self.open.append(op)
        return op

    def radii(self):
        r = eg.radii(self.h)
        return [r[l] for l in range(self.lo, self.hi + 1)]

    def upload(self, fs, vec):
        """a component-major global velocity vector of the top level into three P2 functions"""
        L = self.h.levels[self.hi]
        for k, f in enumerate(fs):
            for c, i in enumerate(self.ids):
                a = np.ascontiguousarray(vec[k * L.n + L.gidx[i]])
                f.upload(self.hi, a[:self.nv], a[self.nv:], cell=c)

    def vector(self, name, vec):
        fs = [self.host.P2Function(self.st, f"{name}{k}", self.lo, self.hi) for k in range(3)]
        self.upload(fs, vec)
        self.open += fs
        return fs

    def read(self, fs):
        L = self.h.levels[self.hi]
        out = np.zeros(3 * L.n)
        for k, f in enumerate(fs):
            for c, i in enumerate(self.ids):
                out[k * L.n + L.gidx[i]] = np.concatenate(f.download(self.hi, cell=c))
        return out

    def close(self):
        for o in self.open[::-1]:
            o.close()
        self.st.close()
