"""GPU tests of the host-layer classes P2ViscousBlockEpsilonOperator, P2P1StokesEpsilonOperator and the solvers instantiated for them
(hyteg_amd/host/p2epsilon.hpp) through hyteg_amd/host.py, against the GLOBAL matrices of tests/p2epsilonutil.py (pinned by
tests/test_p2_epsilon_reference.py; DoFs numbered by physical position, so the shared DoFs of several macro-cells are part of every
comparison), the restated MINRES loop of tests/gmgutil.py and the reference's known answer
(tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp, P2 3-D case)."""
import functools
import time
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import epsilonutil as eu
import gmgutil
import p2divkgradutil as pu
import p2epsilonutil as pe

pytestmark = pytest.mark.gpu
MESHES = Path(__file__).resolve().parent.parent / "hyteg_amd" / "data" / "meshes"
TOL = 1e-12


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


def viscosity(x, y, z):
    """contrast exp( 3 ) * 2 = 40 on the unit cube"""
    return np.exp(3.0 * x) * (1.0 + y)


def field(seed):
    a = np.random.default_rng(seed).uniform(1.0, 4.0, 6)
    return lambda x, y, z: np.sin(a[0] * x + a[1] * y) * np.cos(a[2] * z + a[3]) + 0.3 * np.cos(a[4] * y - a[5] * x)


@functools.lru_cache(maxsize=None)
def restated(mesh, level, stokes=False):
    """the mesh, the viscosity per mesh cell and the global matrix (read-only, shared by the tests)"""
    vertices, cells = (np.asarray(a) for a in gmgutil.mesh(mesh))
    mus = [viscosity(*pu.dof_points(np.asarray(vertices, dtype=np.float64)[cv], level).T) for cv in cells]
    if stokes:
        S, gidx, N, pidx, npr = pe.taylor_hood_matrix(vertices, cells, mus, level)
        return vertices, cells, mus, S, gidx, N, pidx, npr
    A, gidx, N = pe.global_matrix(vertices, cells, mus, level)
    return vertices, cells, mus, A, gidx, N


class Mesh:
    """a host storage with the global numberings of the restatement (the local cells looked up by their mesh cell id)"""

    def __init__(self, env, level, gidx, N, pidx=None, name=None, arrays=None):
        torch, host, hu = env
        self.host, self.hu, self.level, self.N = host, hu, level, N
        if name is not None:
            self.st = host.Storage.from_gmsh(MESHES / f"{name}.msh")
        else:
            self.st = host.Storage.from_arrays(*arrays)
            self.st.set_mesh_boundary_flags_on_boundary(1, 0, True)
        self.st.set_stream(torch.cuda.current_stream().cuda_stream)
        ids = [self.st.local_cell(i)[0] for i in range(self.st.n_local_cells)]
        self.gidx = [gidx[i] for i in ids]
        self.pidx = [pidx[i] for i in ids] if pidx is not None else None
        self.nv = pu.vertex_size(level)

    def upload(self, f, vec):
        """a global vector into a P2Function"""
        for c, g in enumerate(self.gidx):
            a = np.ascontiguousarray(vec[g])
            f.upload(self.level, a[:self.nv], a[self.nv:], cell=c)

    def function(self, name, vec=None):
        f = self.host.P2Function(self.st, name, self.level, self.level)
        if vec is not None:
            self.upload(f, vec)
        return f

    def functions(self, names, vecs):
        return [self.function(n, v) for n, v in zip(names, vecs)]

    def cells_of(self, f):
        return [np.concatenate(f.download(self.level, cell=c)) for c in range(len(self.gidx))]

    def to_global(self, f):
        return pu.to_global(self.gidx, self.N, self.cells_of(f))

    def selection(self, flag, bc=None):
        return [pu.dof_mask(self.level, self.st.mask(i, flag, bc=bc)) for i in range(len(self.gidx))]

    def free(self, flag=None, bc=None):
        free = np.zeros(self.N, dtype=bool)
        sel = self.selection(self.host.Inner | self.host.NeumannBoundary if flag is None else flag, bc)
        for g, s in zip(self.gidx, sel):
            free[g[s]] = True
        for g, s in zip(self.gidx, sel):
            assert np.array_equal(free[g], s)  # every copy of a shared DoF agrees
        return free

    # ---- Taylor-Hood functions: ( u, v, w ) global P2 vectors (3, N) and a global pressure vector (Np,) ----
    def th_function(self, name, uvw, p):
        f = self.host.TaylorHoodFunction(self.st, name, self.level, self.level)
        for k in range(3):
            self.upload(f.velocity[k], uvw[k])
        self.hu.upload(f.pressure, [np.ascontiguousarray(p[ix]) for ix in self.pidx], self.level)
        return f

    def th_global(self, f, npr):
        p = np.zeros(npr)
        for ix, a in zip(self.pidx, self.hu.download(f.pressure, self.level)):
            p[ix] = a
        return np.stack([self.to_global(f.velocity[k]) for k in range(3)]), p

    def close(self):
        self.st.close()


def compare(m, f, want, prior, sels):
    """selected entries of the P2Function f against the global vector at the 1e-12 bar (relative L2 and max entry); the others keep
    `prior` bit for bit"""
    num = den = worst = scale = 0.0
    for got, g, s in zip(m.cells_of(f), m.gidx, sels):
        assert np.array_equal(got[~s], prior[g][~s]), "a DoF the flag excludes was written"
        d = got[s] - want[g][s]
        num, den = num + float(d @ d), den + float(want[g][s] @ want[g][s])
        worst, scale = max(worst, float(np.abs(d).max(initial=0.0))), max(scale, float(np.abs(want[g][s]).max(initial=0.0)))
    assert den > 0.0
    assert np.sqrt(num / den) <= TOL, np.sqrt(num / den)
    assert worst <= TOL * scale, (worst, scale)


@pytest.mark.parametrize("mesh,level", [("cube_6el", 2), ("regular_octahedron_8el", 1)])
def test_apply_and_gemv_against_the_global_matrix(env, mesh, level):
    """flags All and Inner, Replace and Add, gemv with beta != 0 (on several cells through a temporary)"""
    torch, host, hu = env
    vertices, cells, mus, A, gidx, N = restated(mesh, level)
    m = Mesh(env, level, gidx, N, name=mesh)
    pts = pu.global_points(vertices, cells, gidx, N, level)
    src_g = np.stack([field(100 + k)(*pts.T) for k in range(3)])
    prior_g = np.stack([field(110 + k)(*pts.T) for k in range(3)])
    want = (A @ src_g.reshape(3 * N)).reshape(3, N)
    src = m.functions("uvw", src_g)
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    op = host.P2ViscousBlockEpsilonOperator(m.st, level, level, mu)
    for flag in (host.All, host.Inner):
        sels = m.selection(flag)
        shared = sum(int(s.sum()) for s in sels) - len(np.unique(np.concatenate([g[s] for g, s in zip(m.gidx, sels)])))
        assert shared > 0, "the comparison includes DoFs shared between macro-cells"
        dst = m.functions(["du", "dv", "dw"], prior_g)
        op.apply(src, dst, level, flag)
        for k in range(3):
            compare(m, dst[k], want[k], prior_g[k], sels)
        op.apply(src, dst, level, flag, host.Add)
        for k in range(3):
            compare(m, dst[k], 2.0 * want[k], prior_g[k], sels)
        for f in dst:
            f.close()
        alpha, beta = -1.5, 0.25
        dst = m.functions(["du", "dv", "dw"], prior_g)
        op.gemv(alpha, src, beta, dst, level, flag)
        for k in range(3):
            compare(m, dst[k], alpha * want[k] + beta * prior_g[k], prior_g[k], sels)
        for f in dst:
            f.close()
    with pytest.raises(host.HytegHostError, match="dst must differ"):
        op.apply(src, [src[1], src[0], src[2]], level, host.All)
    for o in (op, mu, *src, m):
        o.close()


def test_apply_with_a_neumann_condition_on_w_alone(env):
    """cube_6el, level 2, Inner | NeumannBoundary: u and v under the default condition (flag 1 Dirichlet), w under a condition that makes
    flag 1 a Neumann boundary.  w is written everywhere, u and v at the inner DoFs only: their boundary DoFs stay unwritten"""
    torch, host, hu = env
    mesh, level = "cube_6el", 2
    vertices, cells, mus, A, gidx, N = restated(mesh, level)
    m = Mesh(env, level, gidx, N, name=mesh)
    rng = np.random.default_rng(1100)
    src_g, prior_g = rng.uniform(-1.0, 1.0, (3, N)), rng.uniform(-1.0, 1.0, (3, N))
    want = (A @ src_g.reshape(3 * N)).reshape(3, N)
    src, dst = m.functions("uvw", src_g), m.functions(["du", "dv", "dw"], prior_g)
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    bc = host.BoundaryCondition()
    bc.create_neumann("open", [1])
    dst[2].set_boundary_condition(bc)
    flag = host.Inner | host.NeumannBoundary
    op = host.P2ViscousBlockEpsilonOperator(m.st, level, level, mu)
    op.apply(src, dst, level, flag)
    n_sel = []
    for k in range(3):
        sels = m.selection(flag, bc if k == 2 else None)
        n_sel.append(sum(int(s.sum()) for s in sels))
        compare(m, dst[k], want[k], prior_g[k], sels)
    assert n_sel[0] == n_sel[1] < n_sel[2] == sum(len(g) for g in m.gidx)
    for o in (op, mu, *src, *dst, m):
        o.close()


def test_inverse_diagonal_and_smooth_jac(env):
    """cube_6el, level 2: the inverse diagonals are those of the global matrix's diagonal blocks; smooth_jac is its four statements,
    x + omega D^-1 ( b - A x ) on the selected DoFs"""
    torch, host, hu = env
    mesh, level, omega = "cube_6el", 2, 0.6
    vertices, cells, mus, A, gidx, N = restated(mesh, level)
    m = Mesh(env, level, gidx, N, name=mesh)
    rng = np.random.default_rng(1200)
    x_g, b_g, prior_g = (rng.uniform(-1.0, 1.0, (3, N)) for _ in range(3))
    x, b = m.functions("xyz", x_g), m.functions("abc", b_g)
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    op = host.P2ViscousBlockEpsilonOperator(m.st, level, level, mu)
    with pytest.raises(host.HytegHostError, match="Inverse diagonal values have not been assembled"):
        op.inverse_diagonal()
    op.compute_inverse_diagonal()
    diag = A.diagonal().reshape(3, N)
    everywhere = [np.ones(len(g), dtype=bool) for g in m.gidx]
    for k, f in enumerate(op.inverse_diagonal()):
        compare(m, f, 1.0 / diag[k], prior_g[k], everywhere)
    want = x_g + omega * ((b_g - (A @ x_g.reshape(3 * N)).reshape(3, N)) / diag)
    for flag in (host.Inner, host.All):
        sels = m.selection(flag)
        dst = m.functions(["du", "dv", "dw"], prior_g)
        op.smooth_jac(dst, b, x, omega, level, flag)
        for k in range(3):
            compare(m, dst[k], want[k], prior_g[k], sels)
        for f in dst:
            f.close()
    for o in (op, mu, *x, *b, m):
        o.close()


def stokes_free(m, npr):
    """((3, N), (Np,)) boolean: the DoFs Inner | NeumannBoundary selects (velocity under the default condition, the pressure everywhere)"""
    return np.tile(m.free(), (3, 1)), np.ones(npr, dtype=bool)


def test_stokes_composite_apply(env):
    """TaylorHoodEpsilonStokesOperator.apply equals the restated Taylor-Hood matrix times the vector on cube_6el, level 2,
    Inner | NeumannBoundary: viscOp Replace, divT Add, div Replace"""
    torch, host, hu = env
    mesh, level = "cube_6el", 2
    vertices, cells, mus, S, gidx, N, pidx, npr = restated(mesh, level, True)
    m = Mesh(env, level, gidx, N, pidx, name=mesh)
    rng = np.random.default_rng(1300)
    x_g, prior_g = rng.uniform(-1.0, 1.0, 3 * N + npr), rng.uniform(-1.0, 1.0, 3 * N + npr)
    want = S @ x_g
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    x = m.th_function("x", x_g[:3 * N].reshape(3, N), x_g[3 * N:])
    y = m.th_function("y", prior_g[:3 * N].reshape(3, N), prior_g[3 * N:])
    op = host.TaylorHoodEpsilonStokesOperator(m.st, level, level, mu)
    flag = host.Inner | host.NeumannBoundary
    op.apply(x, y, level, flag)
    sels = m.selection(flag)
    assert 0 < sum(int(s.sum()) for s in sels) < sum(len(s) for s in sels)
    for k in range(3):
        compare(m, y.velocity[k], want[k * N:(k + 1) * N], prior_g[k * N:(k + 1) * N], sels)
    _, p = m.th_global(y, npr)
    assert np.abs(p - want[3 * N:]).max() <= TOL * np.abs(want[3 * N:]).max()
    for o in (op, x, y, mu, m):
        o.close()


@functools.lru_cache(maxsize=None)
def minres_problem():
    """cube_6el, level 2, variable viscosity: a random exact solution, b = S x_exact, a random start"""
    mesh, level = "cube_6el", 2
    vertices, cells, mus, S, gidx, N, pidx, npr = restated(mesh, level, True)
    rng = np.random.default_rng(1400)
    exact = rng.uniform(-1.0, 1.0, 3 * N + npr)
    exact[3 * N:] -= exact[3 * N:].mean()
    b = S @ exact
    x0 = rng.uniform(-1.0, 1.0, 3 * N + npr)
    lumped = pe.lumped_pressure_mass(vertices, cells, level, pidx, npr)
    mu_p = np.zeros(npr)  # the viscosity at the vertex DoFs
    nv = pu.vertex_size(level)
    for ix, mu_c in zip(pidx, mus):
        mu_p[ix] = mu_c[:nv]
    dense = S.toarray()
    for a in (exact, b, x0, lumped, mu_p, dense):
        a.setflags(write=False)
    return mesh, level, exact, b, x0, lumped, mu_p, dense


def restated_minres(free, kind, k, dtype, rel_tol=0.0):
    mesh, level, exact, b, x0, lumped, mu_p, dense = minres_problem()
    n3 = len(exact) - len(lumped)
    start = np.where(free, x0, exact).astype(dtype)
    Sw = dense.astype(dtype)
    scale = np.ones(len(exact), dtype=dtype)
    scale[n3:] = (mu_p if kind == "pressure_viscosity" else 1.0) / lumped
    return gmgutil.minres(lambda u: Sw @ u, lambda r: np.where(free, scale * r, 0), start, b.astype(dtype), free, k, rel_tol)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("kind", ["pressure", "pressure_viscosity"])
def test_minres_iterates_match_the_restated_loop(env, kind, k):
    """x after exactly k iterations against gmgutil.minres on the dense Taylor-Hood matrix, bound gmgutil.tolerance( d ) with d the
    difference between the float64 and the 80-bit run of the restatement"""
    torch, host, hu = env
    mesh, level, exact, b, x0, lumped, mu_p, dense = minres_problem()
    vertices, cells, mus, S, gidx, N, pidx, npr = restated(mesh, level, True)
    m = Mesh(env, level, gidx, N, pidx, name=mesh)
    fv, fp = stokes_free(m, npr)
    free = np.concatenate([fv.reshape(3 * N), fp])
    want, _ = restated_minres(free, kind, k, np.float64)
    wide, _ = restated_minres(free, kind, k, gmgutil.LD)
    bound = gmgutil.tolerance(gmgutil.rel(want, wide))
    start = np.where(free, x0, exact)
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    x = m.th_function("x", start[:3 * N].reshape(3, N), start[3 * N:])
    rhs = m.th_function("b", b[:3 * N].reshape(3, N), b[3 * N:])
    op = host.TaylorHoodEpsilonStokesOperator(m.st, level, level, mu)
    solver = host.TaylorHoodEpsilonSolver.minres(m.st, level, level, max_iter=k, rel_tol=0.0, preconditioner=kind, mu=mu)
    solver.solve(op, x, rhs, level)
    uvw, p = m.th_global(x, npr)
    got = np.concatenate([uvw.reshape(3 * N), p])
    assert np.array_equal(got[~free], start[~free]), "the Dirichlet values are those of the start, bit for bit"
    l2, worst = gmgutil.rel(got, want), float(np.abs(got - want).max() / np.abs(want).max())
    moved = gmgutil.rel(want[free], start[free])
    print(f"{kind} k={k}: relative L2 error {l2:.3e}, largest entry error / max |x| {worst:.3e} (bound {bound:.3e}); moved x by {moved:.2e}")
    assert moved > 1e-3
    assert l2 <= bound and worst <= bound
    for o in (solver, op, x, rhs, mu, m):
        o.close()


def test_cg_on_the_velocity_operator_matches_a_direct_solve(env):
    """cube_6el, level 2, variable viscosity, homogeneous Dirichlet velocity: CGSolver< P2ViscousBlockEpsilonOperator > to 1e-12 ends
    with a relative residual <= 1e-11 on the global matrix and agrees with the sparse direct solve to 1e-7 (condition number times the
    residual: 40 from the viscosity, a few hundred from the P2 element at level 2)"""
    torch, host, hu = env
    mesh, level, tol = "cube_6el", 2, 1e-12
    vertices, cells, mus, A, gidx, N = restated(mesh, level)
    m = Mesh(env, level, gidx, N, name=mesh)
    free = np.tile(m.free(), 3)
    rng = np.random.default_rng(1500)
    b_g = rng.uniform(-1.0, 1.0, 3 * N)
    direct = np.zeros(3 * N)
    direct[free] = spla.spsolve(sp.csc_matrix(A[free][:, free]), b_g[free])
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    x, b = m.functions("xyz", np.zeros((3, N))), m.functions("abc", b_g.reshape(3, N))
    op = host.P2ViscousBlockEpsilonOperator(m.st, level, level, mu)
    cg = host.P2EpsilonSolver.cg(m.st, level, level, max_iter=3000, tol=tol)
    cg.solve(op, x, b, level)
    got = np.concatenate([m.to_global(f) for f in x])
    residual = np.linalg.norm((b_g - A @ got)[free]) / np.linalg.norm(b_g[free])
    print(f"CG: {cg.iterations} iterations, relative residual {residual:.2e}, difference to the direct solve {gmgutil.rel(got, direct):.2e}")
    assert 0 < cg.iterations < 3000
    assert np.array_equal(got[~free], np.zeros(int((~free).sum())))
    assert residual <= 10 * tol
    assert gmgutil.rel(got, direct) <= 1e-7
    for o in (cg, op, mu, *x, *b, m):
        o.close()


def test_jacobi_and_chebyshev_smoothers_reduce_the_residual(env):
    """WeightedJacobiSmoother and ChebyshevSmoother instantiated on the operator as they are: estimateRadius of D^-1 A covers the
    spectrum, and a smoother call from a zero start reduces the energy-norm error"""
    torch, host, hu = env
    mesh, level = "cube_6el", 2
    vertices, cells, mus, A, gidx, N = restated(mesh, level)
    m = Mesh(env, level, gidx, N, name=mesh)
    free = np.tile(m.free(), 3)
    Aff = sp.csc_matrix(A[free][:, free])
    rng = np.random.default_rng(1600)
    exact = np.zeros(3 * N)
    exact[free] = rng.uniform(-1.0, 1.0, int(free.sum()))
    b_g = A @ exact
    mu = m.function("mu", pu.to_global(gidx, N, mus))
    op = host.P2ViscousBlockEpsilonOperator(m.st, level, level, mu)
    op.compute_inverse_diagonal()
    rho = op.estimate_radius(level, 30)
    # estimateRadius iterates on ALL DoFs, as the reference does: against the largest eigenvalue of D^-1 A on all DoFs, which bounds the
    # one on the free DoFs (interlacing).  At most 30: every element matrix has thirty rows.  At least lambda / 1.2: the smoother's
    # default upper bound 1.2 rho must cover the spectrum, or it amplifies
    d = A.diagonal()
    lam = float(spla.eigsh(sp.diags(d ** -0.5) @ A @ sp.diags(d ** -0.5), k=1, which="LA", return_eigenvectors=False)[0])
    print(f"estimated spectral radius {rho:.4f}, largest eigenvalue of D^-1 A {lam:.4f}")
    assert lam / 1.2 <= rho <= 30.0
    b = m.functions("abc", b_g.reshape(3, N))

    def energy_error(fs):
        e = (np.concatenate([m.to_global(f) for f in fs]) - exact)[free]
        return float(np.sqrt(e @ (Aff @ e)))

    start = energy_error(m.functions("000", np.zeros((3, N))))
    for name, solver in (("jacobi", host.P2EpsilonSolver.smoother(m.st, level, level, host.JACOBI, 1.0 / lam)),
                         ("chebyshev", host.P2EpsilonSolver.chebyshev(m.st, level, level, 3, rho))):
        x = m.functions("xyz", np.zeros((3, N)))
        solver.solve(op, x, b, level)
        after = energy_error(x)
        print(f"{name}: energy-norm error {start:.3e} -> {after:.3e}")
        assert after < start  # omega <= 1 / lambda_max: every error component shrinks
        for o in (solver, *x):
            o.close()
    for o in (op, mu, *b, m):
        o.close()


def known_answer(env, level):
    """the reference's P2 3-D case on the cuboid mesh with mu = 1; returns (errors u, v, w, p; iterations; seconds)"""
    torch, host, hu = env
    vertices, cells = eu.cuboid_mesh()
    gidx, N = pu.global_numbering(cells, level)
    pidx, npr = pe.pressure_numbering(gidx, level)
    m = Mesh(env, level, gidx, N, pidx, arrays=(vertices, cells))
    pts = pu.global_points(vertices, cells, gidx, N, level)
    x, y, z = pts.T
    exact = np.stack([eu.known_u(x, y, z), eu.known_v(x, y, z), eu.known_w(x, y, z)])
    dirichlet = ~m.free()
    assert np.array_equal(dirichlet, pe.boundary_dofs(vertices, cells, level, gidx, N))
    mu = m.function("mu", np.ones(N))
    u = m.th_function("u", np.where(dirichlet, exact, 0.0), np.zeros(npr))
    f = m.th_function("f", np.zeros((3, N)), np.zeros(npr))
    mass = host.P2ElementwiseMassOperator(m.st, level, level)
    tmp = m.function("tmp")
    for k, fn in enumerate((eu.known_rhs_u, eu.known_rhs_v, eu.known_rhs_w)):
        m.upload(tmp, fn(x, y, z))
        mass.apply(tmp, f.velocity[k], level, host.All)
    op = host.TaylorHoodEpsilonStokesOperator(m.st, level, level, mu)
    solver = host.TaylorHoodEpsilonSolver.minres(m.st, level, level, max_iter=10000, rel_tol=1e-8, preconditioner="pressure")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.solve(op, u, f, level)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    u.project_pressure_mean(level)
    uvw, p = m.th_global(u, npr)
    pp = np.zeros(npr)
    for c, cv in enumerate(np.asarray(cells, dtype=np.int64)):
        q = pu.dof_points(np.asarray(vertices, dtype=np.float64)[cv], level)[:pu.vertex_size(level)]
        pp[pidx[c]] = eu.known_p(q[:, 0], q[:, 1], q[:, 2])
    pp -= pp.mean()  # projectMean of the exact pressure
    errors = [float(np.sqrt(((uvw[k] - exact[k]) ** 2).sum() / N)) for k in range(3)] + [float(np.sqrt(((p - pp) ** 2).sum() / npr))]
    iterations = solver.minres_iterations
    for o in (solver, op, mass, tmp, u, f, mu, m):
        o.close()
    return errors, iterations, seconds, uvw, p


@pytest.mark.parametrize("level", [2, 3])
def test_known_answer_of_the_reference(env, level):
    """MeshInfo::meshCuboid( (0,0,0), (1,1,1), 1, 1, 1 ), mu = 1, velocity Dirichlet on flag 1, right-hand side through the P2 mass
    operator, MINRES( 10000, 1e-8 ) with the pressure preconditioner (the reference's stokesMinResSolver), projectMean; errors
    sqrt( err . err / DoFs ) under the reference's bounds (level 2: 2.2e-1 / 1.8e+1, level 3: 3.0e-2 / 1.9).  The direct solve on the CPU
    (tests/test_p2_epsilon_reference.py): level 2 u 1.241e-1 v 2.129e-1 w 4.719e-2 p 1.783e+1, level 3 u 1.474e-2 v 2.951e-2 w 6.938e-3
    p 1.873; at level 2 the two solutions are compared as well: the solve stops at a relative residual of 1e-8, and the pressure carries
    the condition of the Schur complement on top of it"""
    errors, iterations, seconds, uvw, p = known_answer(env, level)
    bound_v, bound_p = pe.KNOWN_BOUNDS[level]
    print(f"level {level}: errors u {errors[0]:.3e} v {errors[1]:.3e} w {errors[2]:.3e} (bound {bound_v:.1e}), p {errors[3]:.3e} "
          f"(bound {bound_p:.1e}); {iterations} MINRES iterations in {seconds:.2f} s")
    assert 0 < iterations < 10000
    assert all(0.0 < e < bound_v for e in errors[:3])
    assert 0.0 < errors[3] < bound_p
    if level == 2:
        _, u_cpu, p_cpu, _, _ = pe.known_answer(level)
        print(f"relative difference to the direct solve: velocity {gmgutil.rel(uvw, u_cpu):.2e}, pressure {gmgutil.rel(p, p_cpu):.2e}")
        assert gmgutil.rel(uvw, u_cpu) <= 1e-5 and gmgutil.rel(p, p_cpu) <= 1e-3
