"""GPU tests of the host-layer class P2ElementwiseDivKGrad, of P2ElementwiseMassOperator and of the solvers instantiated for the operator
(hyteg_amd/host/p2divkgrad.hpp, host.P2DivKGradSolver) against the GLOBAL sparse matrices of tests/p2divkgradutil.py -- DoFs numbered by
physical position, so the shared DoFs of several macro-cells are part of every comparison --, against the reference's known answer
(tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp, runAllTestsP2) and against a multigrid cycle restated on the global
matrices (gmgutil.cycle with the quadratic prolongation of p2divkgradutil.prolongation).

Measured rounding d of the restated cycles (float64 against 80-bit, three V(2,2) cycles): printed by test_v_cycle_iterate_by_iterate;
the bound of each comparison is gmgutil.tolerance( d ) = 1e-12 + 50 d."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import gmgutil
import p2divkgradutil as pu
from conftest import REF_TET

pytestmark = pytest.mark.gpu
MESHES = Path(__file__).resolve().parent.parent / "hyteg_amd" / "data" / "meshes"
LD = np.longdouble


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


def field(seed):
    a = np.random.default_rng(seed).uniform(1.0, 4.0, 6)
    return lambda x, y, z: np.sin(a[0] * x + a[1] * y) * np.cos(a[2] * z + a[3]) + 0.3 * np.cos(a[4] * y - a[5] * x)


def coefficient(seed):
    f = field(seed)
    return lambda x, y, z: 1.25 + 0.6 * f(x, y, z)  # within [0.47, 2.03]


class Mesh:
    """a host storage with the global numbering of the restatement: cells in the mesh file's order"""

    def __init__(self, env, name):
        torch, host, hu = env
        self.host = host
        self.st = host.Storage.from_gmsh(MESHES / f"{name}.msh")
        self.st.set_stream(torch.cuda.current_stream().cuda_stream)
        self.vertices, self.cells = (np.asarray(a) for a in gmgutil.mesh(name))
        local = [self.st.local_cell(i) for i in range(self.st.n_local_cells)]
        assert [c[0] for c in local] == list(range(len(self.cells)))
        self.tets = [np.asarray(self.vertices, dtype=np.float64)[cv] for cv in self.cells]
        for (gid, co, nnc), t in zip(local, self.tets):
            assert np.array_equal(np.asarray(co, dtype=np.float64).reshape(4, 3), t)
        self._numbering = {}

    def numbering(self, level):
        if level not in self._numbering:
            self._numbering[level] = pu.global_numbering(self.cells, level)
        return self._numbering[level]

    def interpolate(self, fn, level):
        return [fn(*pu.dof_points(t, level).T) for t in self.tets]

    def to_global(self, arrays, level, dtype=np.float64):
        gidx, ndof = self.numbering(level)
        return pu.to_global(gidx, ndof, arrays, dtype)

    def to_cells(self, u, level):
        return [np.asarray(u[g], dtype=np.float64) for g in self.numbering(level)[0]]

    def selection(self, level, flag, bc=None):
        return [pu.dof_mask(level, self.st.mask(i, flag, bc=bc)) for i in range(len(self.cells))]

    def free(self, level):
        """global mask of the DoFs Inner | NeumannBoundary selects; every copy of a shared DoF agrees"""
        gidx, ndof = self.numbering(level)
        sel = self.selection(level, self.host.Inner | self.host.NeumannBoundary)
        free = np.zeros(ndof, dtype=bool)
        free[np.concatenate([g[s] for g, s in zip(gidx, sel)])] = True
        for g, s in zip(gidx, sel):
            assert np.array_equal(free[g], s)
        return free

    def function(self, name, lo, hi, arrays_by_level=None):
        f = self.host.P2Function(self.st, name, lo, hi)
        for level, arrays in (arrays_by_level or {}).items():
            for c, a in enumerate(arrays):
                nv = pu.vertex_size(level)
                f.upload(level, a[:nv], a[nv:], cell=c)
        return f

    def download(self, f, level):
        return [np.concatenate(f.download(level, cell=c)) for c in range(len(self.cells))]

    def matrix(self, k_arrays, level, dtype=np.float64, mass=False):
        return pu.global_matrix(self.vertices, self.cells, k_arrays, level, dtype, mass)[0]

    def close(self):
        self.st.close()


def rel(a, b):
    a, b = np.concatenate(a), np.concatenate(b)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("mesh,level", [("cube_6el", 2), ("regular_octahedron_8el", 1)])
def test_apply_and_gemv_against_the_global_matrix(env, mesh, level):
    torch, host, hu = env
    m = Mesh(env, mesh)
    u_h, k_h, prior = (m.interpolate(f, level) for f in (field(1), coefficient(2), field(3)))
    u, k = m.function("u", level, level, {level: u_h}), m.function("k", level, level, {level: k_h})
    A = host.P2ElementwiseDivKGrad(m.st, level, level, k)
    G = m.matrix(k_h, level)
    au = m.to_cells(G @ m.to_global(u_h, level), level)
    for flag in (host.All, host.Inner):
        sels = m.selection(level, flag)
        assert any(s.any() for s in sels)
        shared = sum(int(s.sum()) for s in sels) - len(np.unique(np.concatenate([g[s] for g, s in zip(m.numbering(level)[0], sels)])))
        assert shared > 0, "the comparison includes DoFs shared between macro-cells"
        dst = m.function("dst", level, level, {level: prior})
        A.apply(u, dst, level, flag)
        got = m.download(dst, level)
        err = rel([g[s] for g, s in zip(got, sels)], [w[s] for w, s in zip(au, sels)])
        print(f"{mesh} level {level} flag {flag}: apply relative L2 error {err:.3e}")
        assert err <= 1e-12
        for g, p, s in zip(got, prior, sels):
            assert np.array_equal(g[~s], p[~s]), "DoFs the flag does not select keep their contents"
        A.apply(u, dst, level, flag, host.Add)
        got = m.download(dst, level)
        assert rel([g[s] for g, s in zip(got, sels)], [2.0 * w[s] for w, s in zip(au, sels)]) <= 1e-12
        dst.close()
        # gemv with beta != 0: on several cells the shares go through a temporary
        alpha, beta = -1.5, 0.25
        dst = m.function("dst", level, level, {level: prior})
        A.gemv(alpha, u, beta, dst, level, flag)
        got = m.download(dst, level)
        want = [np.where(s, alpha * w + beta * p, p) for w, p, s in zip(au, prior, sels)]
        err = rel([g[s] for g, s in zip(got, sels)], [w[s] for w, s in zip(want, sels)])
        print(f"{mesh} level {level} flag {flag}: gemv relative L2 error {err:.3e}")
        assert err <= 1e-12
        for g, p, s in zip(got, prior, sels):
            assert np.array_equal(g[~s], p[~s])
        dst.close()
    for o in (A, u, k, m):
        o.close()


def test_mass_operator_against_the_global_mass_matrix(env):
    torch, host, hu = env
    level = 2
    m = Mesh(env, "cube_6el")
    u_h = m.interpolate(field(5), level)
    u, dst = m.function("u", level, level, {level: u_h}), m.function("dst", level, level)
    M = host.P2ElementwiseMassOperator(m.st, level, level)
    M.apply(u, dst, level, host.All)
    G = m.matrix(None, level, mass=True)
    assert abs(G.sum() - 1.0) <= 1e-13  # the unit cube
    assert rel(m.download(dst, level), m.to_cells(G @ m.to_global(u_h, level), level)) <= 1e-12
    for o in (M, u, dst, m):
        o.close()


def test_inverse_diagonal_and_smooth_jac(env):
    """the inverse diagonal is that of the global matrix; smooth_jac is its four statements"""
    torch, host, hu = env
    level = 2
    m = Mesh(env, "cube_6el")
    src_h, rhs_h, k_h, prior = (m.interpolate(f, level) for f in (field(51), field(52), coefficient(53), field(54)))
    src, rhs, k = (m.function(n, level, level, {level: a}) for n, a in (("src", src_h), ("rhs", rhs_h), ("k", k_h)))
    A = host.P2ElementwiseDivKGrad(m.st, level, level, k)
    inv = m.function("inv", level, level)
    with pytest.raises(host.HytegHostError, match="Inverse diagonal values have not been assembled"):
        A.smooth_jac(inv, rhs, src, 0.5, level)
    A.compute_inverse_diagonal()
    G = m.matrix(k_h, level)
    A.inverse_diagonal_into(inv, level)
    want_inv = m.to_cells(1.0 / G.diagonal(), level)
    got_inv = m.download(inv, level)
    assert max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got_inv, want_inv)) <= 1e-12
    asrc = m.to_cells(G @ m.to_global(src_h, level), level)
    omega = 0.6
    for flag in (host.Inner, host.All):
        sels = m.selection(level, flag)
        dst = m.function("dst", level, level, {level: prior})
        A.smooth_jac(dst, rhs, src, omega, level, flag)
        got = m.download(dst, level)
        want = [np.where(s, u + omega * (d * (r - a)), p) for s, u, d, r, a, p in zip(sels, src_h, want_inv, rhs_h, asrc, prior)]
        assert rel(got, want) <= 1e-12
        for g, p, s in zip(got, prior, sels):
            assert np.array_equal(g[~s], p[~s])
        dst.close()
    for o in (A, inv, src, rhs, k, m):
        o.close()


def test_boundary_condition_of_the_destination_is_honoured(env):
    """one macro-face carries mesh flag 2: a destination whose own condition makes flag 2 a Neumann boundary gets the DoFs of the face
    written under Inner | NeumannBoundary, one whose condition makes it a Dirichlet boundary does not"""
    torch, host, hu = env
    level = 2
    st = host.Storage.single_tet(REF_TET)
    face = [i for i in range(st.n_faces) if st.primitive(2, i).vertex_ids == (0, 1, 2)]
    st.set_mesh_boundary_flag(2, face[0], 2)
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    tet = np.asarray(REF_TET, dtype=np.float64).reshape(4, 3)
    nv = pu.vertex_size(level)
    u_h, k_h, prior = (f(*pu.dof_points(tet, level).T) for f in (field(31), coefficient(32), field(33)))

    def fun(name, a):
        f = host.P2Function(st, name, level, level)
        f.upload(level, a[:nv], a[nv:])
        return f

    u, k = fun("u", u_h), fun("k", k_h)
    A = host.P2ElementwiseDivKGrad(st, level, level, k)
    flag = host.Inner | host.NeumannBoundary
    ref = pu.apply_cell(u_h, k_h, tet, level)
    on_face = pu.dof_mask(level, 1 << 6)
    assert on_face.any()
    for neumann in (True, False):
        bc = host.BoundaryCondition()
        if neumann:
            bc.create_dirichlet("walls", 1)
            bc.create_neumann("open", [2])
        else:
            bc.create_dirichlet("walls", [1, 2])
        dst = fun("dst", prior)
        dst.set_boundary_condition(bc)
        mask = st.mask(0, flag, bc=bc)
        assert mask == (pu.MASK_INNER | (1 << 6) if neumann else pu.MASK_INNER)
        A.apply(u, dst, level, flag)
        got, sel = np.concatenate(dst.download(level)), pu.dof_mask(level, mask)
        assert np.abs(got[sel] - ref[sel]).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(got[~sel], prior[~sel])
        assert np.array_equal(got[on_face], prior[on_face]) != neumann  # the flagged face was written / was left alone
        dst.close()
    for o in (A, u, k, st):
        o.close()


@pytest.mark.parametrize("level", [2, 3, 4])
def test_known_answer_of_the_reference_by_cg(env, level):
    """tet_1el, levels 2, 3, 4: right-hand side through P2ElementwiseMassOperator, CGSolver( 1000, 1e-12 ); the error is inside the
    reference's bounds 4.5e-3, 4.6e-4, 3.8e-5 and agrees with the direct solve of the restatement to 1e-6 relative"""
    torch, host, hu = env
    m = Mesh(env, "tet_1el")
    tet = tuple(map(tuple, m.tets[0]))  # the mesh file's node order
    k = m.function("k", level, level, {level: m.interpolate(pu.known_k, level)})
    r = m.function("r", level, level, {level: m.interpolate(pu.known_rhs, level)})
    f = m.function("f", level, level)
    M = host.P2ElementwiseMassOperator(m.st, level, level)
    M.apply(r, f, level, host.All)
    exact = m.interpolate(pu.known_u, level)[0]
    inner = m.selection(level, host.Inner)[0]
    u = m.function("u", level, level, {level: [np.where(inner, 0.0, exact)]})
    A = host.P2ElementwiseDivKGrad(m.st, level, level, k)
    cg = host.P2DivKGradSolver.cg(m.st, level, level, max_iter=1000, tol=1e-12)
    cg.solve(A, u, f, level)
    err = pu.known_error(m.download(u, level)[0], level, tet)
    cpu = pu.known_answer(level, tet)[0]
    print(f"level {level}: {pu.size(level)} DoFs, error {err:.6e} (restatement {cpu:.6e}, bound {pu.KNOWN_BOUNDS[level]:.1e}), {cg.iterations} CG iterations")
    assert 0 < cg.iterations < 1000
    assert err < pu.KNOWN_BOUNDS[level]
    assert abs(err - cpu) <= 1e-6 * cpu
    for o in (cg, A, M, u, f, r, k, m):
        o.close()


# ---- the multigrid cycle restated on global matrices ----
class Level:
    def __init__(self, A, free, level):
        self.A, self.free, self.level = sp.csr_matrix(A), free, level
        self.D, self._wide = self.A.diagonal(), None

    def matrix(self, dtype):
        if dtype == np.float64:
            return self.A
        if self._wide is None:
            self._wide = self.A.astype(LD)
        return self._wide

    def apply(self, u):
        return self.matrix(u.dtype) @ u


def hierarchy(m, lo, hi, k_fn):
    h = object.__new__(gmgutil.Hierarchy)
    h.lo, h.hi, h._P_wide = lo, hi, {}
    h.levels = {l: Level(m.matrix(m.interpolate(k_fn, l), l), m.free(l), l) for l in range(lo, hi + 1)}
    h.P = {l: pu.prolongation(l, *m.numbering(l), *m.numbering(l + 1)) for l in range(lo, hi)}
    return h


CYCLES = 3


def run_cycles(h, x0, b0, dtype):
    smoother = gmgutil.jacobi_smoother(h, 2.0 / 3.0)
    xs = {l: np.zeros(h.levels[l].A.shape[0], dtype=dtype) for l in range(h.lo, h.hi + 1)}
    bs = {l: np.zeros(h.levels[l].A.shape[0], dtype=dtype) for l in range(h.lo, h.hi + 1)}
    xs[h.hi], bs[h.hi] = x0.astype(dtype), b0.astype(dtype)
    out = []
    for _ in range(CYCLES):
        gmgutil.cycle(h, smoother, xs, bs, h.hi, 2, 2)
        out.append(xs[h.hi].copy())
    return out


@pytest.mark.parametrize("mesh", ["tet_1el", "cube_6el"])
def test_v_cycle_iterate_by_iterate(env, mesh):
    """V( 2, 2 ) with Jacobi( 2 / 3 ), levels 2-3, exact coarse solve: the iterates of GeometricMultigridSolver against the restated cycle
    (P: the coarse P2 basis at the fine DoFs, restriction P^T on the free DoFs), bound 1e-12 + 50 d with d measured between the float64
    and the 80-bit restatement"""
    torch, host, hu = env
    lo, hi = 2, 3
    m = Mesh(env, mesh)
    kf = coefficient(7)
    h = hierarchy(m, lo, hi, kf)
    free = h.levels[hi].free
    rng = np.random.default_rng(17)
    n = len(free)
    x0, b0 = np.where(free, rng.uniform(-1.0, 1.0, n), 0.0), np.where(free, rng.uniform(-1.0, 1.0, n), 0.0)
    want, wide = run_cycles(h, x0, b0, np.float64), run_cycles(h, x0, b0, LD)
    d = max(gmgutil.rel(a, w) for a, w in zip(want, wide))
    k = m.function("k", lo, hi, {l: m.interpolate(kf, l) for l in range(lo, hi + 1)})
    zeros = {l: [np.zeros(pu.size(l))] * len(m.cells) for l in range(lo, hi)}
    x = m.function("x", lo, hi, {**zeros, hi: m.to_cells(x0, hi)})
    b = m.function("b", lo, hi, {**zeros, hi: m.to_cells(b0, hi)})
    A = host.P2ElementwiseDivKGrad(m.st, lo, hi, k)
    A.compute_inverse_diagonal()
    gmg = host.P2DivKGradSolver.gmg(m.st, lo, hi, smoother=host.JACOBI, relax=2.0 / 3.0, pre=2, post=2)
    for it in range(CYCLES):
        gmg.solve(A, x, b, hi)
        got = m.to_global(m.download(x, hi), hi)
        err = gmgutil.rel(got, want[it])
        print(f"{mesh} cycle {it + 1}: relative L2 difference {err:.3e}, measured rounding d {d:.3e}, bound {gmgutil.tolerance(d):.3e}")
        assert err <= gmgutil.tolerance(d)
    for o in (gmg, A, x, b, k, m):
        o.close()


def test_multigrid_preconditioned_cg_needs_fewer_iterations(env):
    """cube_6el, levels 2-3: CG preconditioned by one V( 2, 2 ) Jacobi cycle against plain CG, both to 1e-10 (counts: DESIGN.md 3.19)"""
    torch, host, hu = env
    lo, hi, tol = 2, 3, 1e-10
    m = Mesh(env, "cube_6el")
    kf = coefficient(7)
    k_h = {l: m.interpolate(kf, l) for l in range(lo, hi + 1)}
    k = m.function("k", lo, hi, k_h)
    G, free = m.matrix(k_h[hi], hi), m.free(hi)
    b0 = np.where(free, m.to_global(m.interpolate(field(9), hi), hi), 0.0)
    zeros = {l: [np.zeros(pu.size(l))] * len(m.cells) for l in range(lo, hi + 1)}
    b = m.function("b", lo, hi, {**zeros, hi: m.to_cells(b0, hi)})
    A = host.P2ElementwiseDivKGrad(m.st, lo, hi, k)
    A.compute_inverse_diagonal()
    gmg = host.P2DivKGradSolver.gmg(m.st, lo, hi, smoother=host.JACOBI, relax=2.0 / 3.0, pre=2, post=2)
    pcg = host.P2DivKGradSolver.cg(m.st, lo, hi, max_iter=200, tol=tol, preconditioner=gmg)
    cg = host.P2DivKGradSolver.cg(m.st, hi, hi, max_iter=2000, tol=tol)
    res = {}
    for name, solver in (("pcg", pcg), ("cg", cg)):
        x = m.function("x", lo, hi, zeros)
        solver.solve(A, x, b, hi)
        xg = m.to_global(m.download(x, hi), hi)
        res[name] = (np.linalg.norm((b0 - G @ xg)[free]) / np.linalg.norm(b0[free]), xg)
        x.close()
    print(f"preconditioned CG {pcg.iterations} iterations (residual {res['pcg'][0]:.2e}), plain CG {cg.iterations} ({res['cg'][0]:.2e})")
    assert res["pcg"][0] <= 10 * tol and res["cg"][0] <= 10 * tol
    assert gmgutil.rel(res["pcg"][1], res["cg"][1]) <= 1e-7
    assert 0 < pcg.iterations < cg.iterations < 2000
    for o in (pcg, cg, gmg, A, b, k, m):
        o.close()


def test_chebyshev_smoother_and_full_multigrid_reduce_the_residual(env):
    """tet_1el, levels 2-3: estimateRadius of D^-1 A lies in ( 0, 10 ] (ten DoFs per element); V( 1, 1 ) cycles with ChebyshevSmoother( 2 )
    at least halve the residual of the global matrix, cycle by cycle (a working cycle contracts by a level-independent factor well below
    one; a wrong transfer, diagonal or radius stalls near one or diverges); FullMultigridSolver with two such cycles per level ends below
    the residual one cycle from zero reaches"""
    torch, host, hu = env
    lo, hi = 2, 3
    m = Mesh(env, "tet_1el")
    kf = coefficient(7)
    k_h = {l: m.interpolate(kf, l) for l in range(lo, hi + 1)}
    k = m.function("k", lo, hi, k_h)
    G, free = m.matrix(k_h[hi], hi), m.free(hi)
    b0 = np.where(free, m.to_global(m.interpolate(field(9), hi), hi), 0.0)
    zeros = {l: [np.zeros(pu.size(l))] * len(m.cells) for l in range(lo, hi + 1)}
    A = host.P2ElementwiseDivKGrad(m.st, lo, hi, k)
    A.compute_inverse_diagonal()
    radii = []
    for l in range(lo, hi + 1):
        v, t = m.function("v", l, l, {l: m.interpolate(lambda x, y, z: 1.0 + np.sin(5 * x + y) * np.cos(3 * z), l)}), m.function("t", l, l)
        radii.append(host.estimate_radius(A, l, 30, v, t))
        v.close(), t.close()
    print("spectral radii of D^-1 A:", radii)
    assert all(0.0 < r <= 10.0 for r in radii)
    residual = lambda f: float(np.linalg.norm((b0 - G @ m.to_global(m.download(f, hi), hi))[free]) / np.linalg.norm(b0[free]))  # noqa: E731
    gmg = host.P2DivKGradSolver.gmg_chebyshev(m.st, lo, hi, 2, radii, pre=1, post=1)
    b, x = m.function("b", lo, hi, {**zeros, hi: m.to_cells(b0, hi)}), m.function("x", lo, hi, zeros)
    res = [1.0]
    for _ in range(3):
        gmg.solve(A, x, b, hi)
        res.append(residual(x))
    print("residual after each Chebyshev( 2 ) V( 1, 1 ) cycle:", res[1:])
    assert all(b_ < 0.5 * a_ for a_, b_ in zip(res, res[1:]))
    fmg = host.P2DivKGradSolver.fmg(m.st, gmg, lo, hi, cycles_per_level=2)
    y = m.function("y", lo, hi, zeros)
    b2 = m.function("b2", lo, hi, {**zeros, hi: m.to_cells(b0, hi)})
    fmg.solve(A, y, b2, hi)
    print("residual after full multigrid:", residual(y))
    assert residual(y) < res[1]
    cheb = host.P2DivKGradSolver.chebyshev(m.st, hi, hi, 3, radii[-1])
    z = m.function("z", hi, hi, {hi: zeros[hi]})
    cheb.solve(A, z, b, hi)
    assert residual(z) < 1.0
    for o in (cheb, fmg, gmg, A, x, y, z, b, b2, k, m):
        o.close()
