"""GPU tests of MINRES on the Taylor-Hood epsilon Stokes operator with the block-diagonal preconditioners "block" and "block_viscosity"
(host.TaylorHoodEpsilonSolver.minres: StokesVectorBlockDiagonalPreconditioner, whose velocity action is one V( 1, 1 ) Chebyshev( 2 )
cycle on P2ViscousBlockEpsilonOperator) against the restated loop of tests/p2epsilongmgutil.py on the dense Taylor-Hood matrix.  The
problem: cube_6el, level 2, mu = exp( 3 x )( 1 + y ) (tests/test_p2_epsilon_gmg_restatement.py); the velocity cycle runs on the levels 1-2
on both sides.  Bound of the iterates: gmgutil.tolerance( d ), d the restatement's own float64-against-80-bit difference."""
import numpy as np
import pytest

import gmgutil as gm
import p2divkgradutil as pu
import p2epsilongmgutil as pg
import p2epsilonutil as pe
import test_gpu_p2_epsilon_host as base  # its Mesh and known-answer set-up; no test of it is imported by name

pytestmark = pytest.mark.gpu
MESH, LO, HI = "cube_6el", 1, 2


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


class Stokes:
    """the device side of p2epsilongmgutil.stokes_problem: Taylor-Hood functions over the levels LO..HI filled on the top level"""

    def __init__(self, env):
        torch, host, hu = env
        self.host, self.hu = host, hu
        self.dev = pg.Device(host, hu, torch.cuda.current_stream().cuda_stream, MESH, LO, HI)
        self.p = pg.stokes_problem(MESH, LO, HI)
        self.n3 = len(self.p["free"]) - self.p["npr"]
        self.op = host.TaylorHoodEpsilonStokesOperator(self.dev.st, LO, HI, self.dev.mu)
        self.open = [self.op]

    def function(self, name, vec):
        f = self.host.TaylorHoodFunction(self.dev.st, name, LO, HI)
        self.dev.upload(f.velocity, vec[:self.n3])
        self.hu.upload(f.pressure, [np.ascontiguousarray(vec[self.n3:][self.p["pidx"][i]]) for i in self.dev.ids], HI)
        self.open.append(f)
        return f

    def read(self, f):
        p = np.zeros(self.p["npr"])
        for i, a in zip(self.dev.ids, self.hu.download(f.pressure, HI)):
            p[self.p["pidx"][i]] = a
        return np.concatenate([self.dev.read(f.velocity), p])

    def solver(self, kind, max_iter, rel_tol, **kw):
        s = self.host.TaylorHoodEpsilonSolver.minres(self.dev.st, LO, HI, max_iter=max_iter, rel_tol=rel_tol, preconditioner=kind, mu=self.dev.mu,
                                                     radii=self.dev.radii() if kind.startswith("block") else None, **kw)
        self.open.append(s)
        return s

    def close(self):
        for o in self.open[::-1]:
            o.close()
        self.dev.close()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("kind", ["block", "block_viscosity"])
def test_minres_iterates_match_the_restated_loop(env, kind, k):
    s = Stokes(env)
    want, _ = pg.minres(MESH, LO, HI, kind, k)
    wide, _ = pg.minres(MESH, LO, HI, kind, k, dtype=gm.LD)
    bound = gm.tolerance(gm.rel(want, wide))
    free, start = s.p["free"], s.p["start"]
    x, rhs = s.function("x", start), s.function("b", s.p["b"])
    s.solver(kind, k, 0.0).solve(s.op, x, rhs, HI)
    got = s.read(x)
    assert np.array_equal(got[~free], start[~free]), "the Dirichlet values are those of the start, bit for bit"
    l2, worst = gm.rel(got, want), float(np.abs(got - want).max() / np.abs(want).max())
    moved = gm.rel(want[free], start[free])
    print(f"{kind} k={k}: relative L2 error {l2:.3e}, largest entry error / max |x| {worst:.3e} (bound {bound:.3e}); moved x by {moved:.2e}")
    assert moved > 1e-3
    assert l2 <= bound and worst <= bound
    s.close()


def test_block_needs_fewer_iterations_than_pressure_and_as_many_as_the_restated_loop(env):
    """iterations to 1e-8: "block" within one of the restated loop's count, and strictly below the "pressure" count of the same run"""
    s = Stokes(env)
    _, etas = pg.minres(MESH, LO, HI, "block", 3000, rel_tol=1e-8)
    counts = {}
    for kind in ("block", "pressure"):
        x, rhs = s.function("x" + kind, s.p["start"]), s.function("b" + kind, s.p["b"])
        solver = s.solver(kind, 3000, 1e-8)
        solver.solve(s.op, x, rhs, HI)
        counts[kind] = solver.minres_iterations
    restated = len(etas) - 1  # getIterations: the index of the iteration that met the tolerance
    print(f"MINRES to 1e-8: block {counts['block']} (restated loop {restated}), pressure {counts['pressure']} iterations")
    assert abs(counts["block"] - restated) <= 1
    assert 0 < counts["block"] < counts["pressure"] < 3000
    s.close()


def test_known_answer_with_the_block_preconditioner(env):
    """the reference's P2 3-D case on the cuboid mesh (p2epsilonutil.known_answer, mu = 1) at level 2 with "block", velocity cycle on the
    levels 1-2: the errors lie inside the reference's bounds 2.2e-1 / 1.8e+1"""
    torch, host, hu = env
    level, lo = 2, 1
    vertices, cells = base.eu.cuboid_mesh()
    gidx, N = pu.global_numbering(cells, level)
    pidx, npr = pe.pressure_numbering(gidx, level)
    m = base.Mesh(env, level, gidx, N, pidx, arrays=(vertices, cells))
    pts = pu.global_points(vertices, cells, gidx, N, level)
    x, y, z = pts.T
    exact = np.stack([base.eu.known_u(x, y, z), base.eu.known_v(x, y, z), base.eu.known_w(x, y, z)])
    dirichlet = ~m.free()
    mu = host.P2Function(m.st, "mu", lo, level)
    for l in range(lo, level + 1):
        mu.interpolate(1.0, l, host.All)

    def th(name, uvw):
        f = host.TaylorHoodFunction(m.st, name, lo, level)
        for k in range(3):
            m.upload(f.velocity[k], uvw[k])
        return f

    u, f = th("u", np.where(dirichlet, exact, 0.0)), th("f", np.zeros((3, N)))
    mass = host.P2ElementwiseMassOperator(m.st, level, level)
    tmp = m.function("tmp")
    for k, fn in enumerate((base.eu.known_rhs_u, base.eu.known_rhs_v, base.eu.known_rhs_w)):
        m.upload(tmp, fn(x, y, z))
        mass.apply(tmp, f.velocity[k], level, host.All)
    op = host.TaylorHoodEpsilonStokesOperator(m.st, lo, level, mu)
    solver = host.TaylorHoodEpsilonSolver.minres(m.st, lo, level, max_iter=10000, rel_tol=1e-8, preconditioner="block", mu=mu)
    solver.solve(op, u, f, level)
    u.project_pressure_mean(level)
    uvw, p = m.th_global(u, npr)
    pp = np.zeros(npr)
    for c, cv in enumerate(np.asarray(cells, dtype=np.int64)):
        q = pu.dof_points(np.asarray(vertices, dtype=np.float64)[cv], level)[:pu.vertex_size(level)]
        pp[pidx[c]] = base.eu.known_p(q[:, 0], q[:, 1], q[:, 2])
    pp -= pp.mean()
    errors = [float(np.sqrt(((uvw[k] - exact[k]) ** 2).sum() / N)) for k in range(3)] + [float(np.sqrt(((p - pp) ** 2).sum() / npr))]
    bound_v, bound_p = pe.KNOWN_BOUNDS[level]
    print(f"level {level} block: errors u {errors[0]:.3e} v {errors[1]:.3e} w {errors[2]:.3e} (bound {bound_v:.1e}), p {errors[3]:.3e} "
          f"(bound {bound_p:.1e}); {solver.minres_iterations} MINRES iterations")
    assert 0 < solver.minres_iterations < 10000
    assert all(0.0 < e < bound_v for e in errors[:3]) and 0.0 < errors[3] < bound_p
    for o in (solver, op, mass, tmp, u, f, mu, m):
        o.close()


def test_an_unsymmetric_configuration_raises(env):
    """MINRES needs a symmetric positive definite preconditioner: pre != post, a Gauss-Seidel smoother and a loose coarse solve are refused"""
    torch, host, hu = env
    s = Stokes(env)
    for kw in (dict(pre=1, post=2), dict(smoother="gauss_seidel"), dict(cg_tol=1e-6)):
        with pytest.raises(host.HytegHostError):
            s.solver("block", 10, 1e-8, **kw)
    with pytest.raises(host.HytegHostError, match="needs mu"):
        host.TaylorHoodEpsilonSolver.minres(s.dev.st, LO, HI, preconditioner="block")
    s.close()
