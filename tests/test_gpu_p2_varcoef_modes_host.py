"""GPU tests of the fused steps of the host-layer classes P2ViscousBlockEpsilonOperator and P2ElementwiseDivKGrad
(hyteg_amd/host/p2epsilon.hpp, p2divkgrad.hpp, schedule: p2varcoefsteps.hpp) through hyteg_amd/host.py: residual, smooth_jac and a
ChebyshevSmoother call of orders 1, 2 and 3, fused against composed (set_fused( False )) and against the GLOBAL matrices of
tests/p2epsilonutil.py / tests/p2divkgradutil.py (DoFs numbered by physical position: the shared DoFs of several macro-cells are part of
every comparison).  cube_6el level 2 and regular_octahedron_8el level 1, mu = exp( 3 x )( 1 + y ) (contrast 40).  Bound: 1e-12 relative
L2 per component; DoFs a component's condition excludes keep their contents bit for bit."""
import functools

import numpy as np
import pytest

import chebyshevutil as cu
import p2divkgradutil as pu
import test_gpu_p2_epsilon_host as base  # its Mesh, restated meshes and viscosity; no test of it is imported by name

pytestmark = pytest.mark.gpu
TOL = 1e-12
CASES = [("cube_6el", 2), ("regular_octahedron_8el", 1)]
OPS = ["epsilon", "divkgrad"]
RHO = 3.4  # a spectral radius for the coefficients; the comparison does not depend on its quality


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


@functools.lru_cache(maxsize=None)
def matrices(mesh, level):
    """( global epsilon matrix (3 N, 3 N), global div-k-grad matrix (N, N) with k = mu, numbering, N, mu per cell ): read-only"""
    vertices, cells, mus, A, gidx, N = base.restated(mesh, level)
    return A, pu.global_matrix(vertices, cells, mus, level)[0], gidx, N, mus


class Problem:
    """an operator of either kind on a mesh with its global matrix; vectors are (nc, N) global arrays, functions lists of nc P2Functions"""

    def __init__(self, env, op, mesh, level, bcs=None):
        torch, host, hu = env
        A3, A1, gidx, N, mus = matrices(mesh, level)
        self.host, self.op_name, self.level, self.N = host, op, level, N
        self.nc = 3 if op == "epsilon" else 1
        self.A = A3 if op == "epsilon" else A1
        self.m = base.Mesh(env, level, gidx, N, name=mesh)
        self.mu = self.m.function("mu", pu.to_global(gidx, N, mus))
        cls = host.P2ViscousBlockEpsilonOperator if op == "epsilon" else host.P2ElementwiseDivKGrad
        self.op = cls(self.m.st, level, level, self.mu)
        self.op.compute_inverse_diagonal()
        self.inv = 1.0 / self.A.diagonal().reshape(self.nc, N)
        self.bcs = bcs or [None] * self.nc
        self.flag = host.Inner | host.NeumannBoundary
        self.sels = [self.m.selection(self.flag, bc) for bc in self.bcs]  # per component, per cell
        self.free = np.stack([self.m.free(self.flag, bc) for bc in self.bcs])
        self.open = [self.op, self.mu]

    def functions(self, name, vec):
        fs = [self.m.function(f"{name}{k}", vec[k]) for k in range(self.nc)]
        for f, bc in zip(fs, self.bcs):
            if bc is not None:
                f.set_boundary_condition(bc)
        self.open += fs
        return fs

    def arg(self, fs):
        return fs if self.op_name == "epsilon" else fs[0]

    def apply(self, v):
        return (self.A @ v.reshape(self.nc * self.N)).reshape(self.nc, self.N)

    def check(self, fs, want, prior, what):
        for k in range(self.nc):
            num = den = 0.0
            for got, g, s in zip(self.m.cells_of(fs[k]), self.m.gidx, self.sels[k]):
                assert np.array_equal(got[~s], prior[k][g][~s]), f"{what}: component {k}: a DoF its condition excludes was written"
                d = got[s] - want[k][g][s]
                num, den = num + float(d @ d), den + float(want[k][g][s] @ want[k][g][s])
            if den == 0.0:
                assert num == 0.0
                continue
            print(f"{what} component {k}: relative L2 error {np.sqrt(num / den):.2e}")
            assert np.sqrt(num / den) <= TOL, (what, k, np.sqrt(num / den))

    def chebyshev(self, order):
        solver = self.host.P2EpsilonSolver if self.op_name == "epsilon" else self.host.P2DivKGradSolver
        s = solver.chebyshev(self.m.st, self.level, self.level, order, RHO)
        self.open.append(s)
        return s

    def close(self):
        for o in self.open[::-1]:
            o.close()
        self.m.close()


def run_all(p, seed, fused):
    """residual, smooth_jac and Chebyshev( 1, 2, 3 ) with the operator's switch at `fused`; returns what each wrote, after checking it
    against the global matrix"""
    rng = np.random.default_rng(seed)
    x_g, b_g, prior_g = (rng.uniform(-1.0, 1.0, (p.nc, p.N)) for _ in range(3))
    x, b = p.functions("x", x_g), p.functions("b", b_g)
    p.op.set_fused(fused)
    assert p.op.chebyshev_fusable(p.level) == fused
    out = {}
    r = p.functions("r", prior_g)
    p.op.residual(p.arg(x), p.arg(b), p.arg(r), p.level, p.flag)
    p.check(r, b_g - p.apply(x_g), prior_g, f"residual fused={fused}")
    out["residual"] = r
    d = p.functions("d", prior_g)
    p.op.smooth_jac(p.arg(d), p.arg(b), p.arg(x), 0.6, p.level, p.flag)
    p.check(d, x_g + 0.6 * (p.inv * (b_g - p.apply(x_g))), prior_g, f"smooth_jac fused={fused}")
    out["smooth_jac"] = d
    for order in (1, 2, 3):
        c = cu.coefficients(order, 0.3 * RHO, 1.2 * RHO)
        # the smoother's sequence on the free DoFs (its temporaries are zero elsewhere): t = D^-1 ( b - A x ); x += c0 t; t = D^-1 A t; ...
        t = np.where(p.free, p.inv * (b_g - p.apply(x_g)), 0.0)
        want = x_g + c[0] * t
        for k in range(1, order):
            t = np.where(p.free, p.inv * p.apply(t), 0.0)
            want = want + c[k] * t
        y = p.functions(f"y{order}", x_g)
        p.chebyshev(order).solve(p.op, p.arg(y), p.arg(b), p.level)
        p.check(y, want, x_g, f"chebyshev({order}) fused={fused}")
        out[f"chebyshev{order}"] = y
    return out


def fused_against_composed(p):
    fused, composed = run_all(p, 77, True), run_all(p, 77, False)
    for what in fused:
        for k in range(p.nc):
            a = np.concatenate(p.m.cells_of(fused[what][k]))
            b = np.concatenate(p.m.cells_of(composed[what][k]))
            rel = np.linalg.norm(a - b) / np.linalg.norm(b)
            print(f"{what} component {k}: fused against composed, relative L2 {rel:.2e}")
            assert rel <= TOL, (what, k, rel)


@pytest.mark.parametrize("mesh,level", CASES)
@pytest.mark.parametrize("op", OPS)
def test_fused_steps_against_composed_and_the_global_matrix(env, op, mesh, level):
    p = Problem(env, op, mesh, level)
    shared = sum(int(s.sum()) for s in p.sels[0]) - int(p.free[0].sum())
    assert shared > 0, "the comparison includes DoFs shared between macro-cells"
    fused_against_composed(p)
    p.close()


def test_a_neumann_condition_on_w_alone_stays_on_the_fused_path(env):
    """cube_6el level 2: u and v under the default condition, w under one that makes flag 1 a Neumann boundary: w is written everywhere,
    u and v at the inner DoFs only, by the fused steps (chebyshev_fusable stays true: run_all asserts it)"""
    torch, host, hu = env
    bc = host.BoundaryCondition()
    bc.create_neumann("open", [1])
    p = Problem(env, "epsilon", "cube_6el", 2, bcs=[None, None, bc])
    assert p.free[0].sum() == p.free[1].sum() < p.free[2].sum() == p.N
    fused_against_composed(p)
    p.close()


def test_a_component_fixed_everywhere_is_not_written(env):
    """v under a condition that makes every primitive a Dirichlet boundary: no step writes it"""
    torch, host, hu = env
    bc = host.BoundaryCondition()
    bc.create_dirichlet("fixed", [0, 1])
    p = Problem(env, "epsilon", "cube_6el", 2, bcs=[None, bc, None])
    assert p.free[1].sum() == 0 < p.free[0].sum()
    fused_against_composed(p)
    p.close()
