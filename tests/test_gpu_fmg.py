"""FullMultigridSolver through the host layer (src/hyteg/solvers/FullMultigridSolver.hpp:33-114): a full multigrid pass is the
sequence `cycles_per_level[l]` multigrid cycles on level l, then the FMG prolongation to level l + 1, for l = min .. max -- so it
must leave x on every level bit-identical to that sequence issued by hand through the entry points that existed before."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
MESHES = ROOT / "hyteg_amd" / "data" / "meshes"
LO, HI = 2, 4


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host


def _fmg_flag(host):
    return host.Inner | host.NeumannBoundary | host.FreeslipBoundary


class _P1Problem:
    """-laplace u = 1 with u = 0 on the boundary, V(2,2) Jacobi cycles, CG on the coarsest level"""

    def __init__(self, torch, host, mesh, graphs):
        self.host = host
        self.st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
        self.st.set_stream(torch.cuda.current_stream().cuda_stream)
        self.A = host.P1ConstantOperator(self.st, LO, HI)
        self.A.compute_inverse_diagonal()
        self.x, self.b, self.r = (host.P1Function(self.st, n, LO, HI) for n in ("x", "b", "r"))
        self.gmg = host.Solver.gmg(self.st, LO, HI, smoother=host.JACOBI, relax=2.0 / 3.0, pre=2, post=2, cg_max_iter=200, cg_tol=1e-13)
        self.gmg.set_use_graphs(graphs)

    def reset(self):
        # a cycle on level l overwrites b on the levels below: set the right-hand side of every level again
        for level in range(LO, HI + 1):
            self.x.interpolate(0.0, level)
            self.b.interpolate(0.0, level)
            self.b.interpolate(1.0, level, self.host.Inner)

    def iterate(self):
        return [[self.x.download_cell(c, level) for c in range(self.st.n_local_cells)] for level in range(LO, HI + 1)]

    def residual_norm(self):
        host = self.host
        self.r.interpolate(0.0, HI)
        self.A.apply(self.x, self.r, HI, host.Inner)
        self.r.assign([1.0, -1.0], [self.b, self.r], HI, host.Inner)
        return float(np.sqrt(self.r.dot(self.r, HI, host.Inner)))


def _by_hand(p, host, cycles, prolongation):
    for level in range(LO, HI + 1):
        for _ in range(cycles[level]):
            p.gmg.solve(p.A, p.x, p.b, level)
        if level < HI:
            if prolongation == "linear":
                host.prolongate(p.x, level, _fmg_flag(host))
            else:
                host.prolongate_quadratic(p.x, level, _fmg_flag(host))


@pytest.mark.parametrize("mesh", ["tet_1el", "cube_6el"])
@pytest.mark.parametrize("prolongation", ["linear", "quadratic"])
@pytest.mark.parametrize("cycles", [1, [9, 9, 2, 1, 3]], ids=["one cycle per level", "cycles per level"])
@pytest.mark.parametrize("graphs", [False, True], ids=["launches", "graphs"])
def test_fmg_is_the_sequence_issued_by_hand(env, mesh, prolongation, cycles, graphs):
    torch, capi, host = env
    per_level = [cycles] * (HI + 1) if isinstance(cycles, int) else cycles
    hand, auto = _P1Problem(torch, host, mesh, graphs), _P1Problem(torch, host, mesh, graphs)
    fmg = host.Solver.fmg(auto.st, auto.gmg, LO, HI, cycles_per_level=cycles, prolongation=prolongation)
    # three passes: with graphs the first runs ordinary launches, the second records and replays, the third replays
    for _ in range(3 if graphs else 1):
        hand.reset()
        auto.reset()
        _by_hand(hand, host, per_level, prolongation)
        fmg.solve(auto.A, auto.x, auto.b, HI)
        for want, got in zip(hand.iterate(), auto.iterate()):
            for w, g in zip(want, got):
                assert np.array_equal(w, g)
    assert (auto.gmg.replayed_cycles > 0) == graphs
    assert max(np.abs(a).max() for a in auto.iterate()[-1]) > 0.0


def test_callbacks_arrive_in_the_reference_order_and_the_residual_falls(env):
    torch, capi, host = env
    p = _P1Problem(torch, host, "cube_6el", False)
    seen = []
    fmg = host.Solver.fmg(p.st, p.gmg, LO, HI, cycles_per_level=1, prolongation="quadratic",
                          post_cycle=lambda level: seen.append(("cycle", level)), post_prolongate=lambda level: seen.append(("prolongate", level)))
    p.reset()
    start = p.residual_norm()
    fmg.solve(p.A, p.x, p.b, HI)
    # the post-prolongate callback also arrives on the top level, where nothing is prolongated (FullMultigridSolver.hpp:109-111)
    assert seen == [(what, level) for level in range(LO, HI + 1) for what in ("cycle", "prolongate")]
    after = p.residual_norm()
    print(f"residual norm on level {HI}: zero start {start:.6e}, after one FMG pass {after:.6e}")
    assert after < start
    # solve( level ) below the top level stops there, and still prolongates to the next level
    del seen[:]
    p.reset()
    fmg.solve(p.A, p.x, p.b, LO + 1)
    assert seen == [(what, level) for level in (LO, LO + 1) for what in ("cycle", "prolongate")]
    assert np.abs(p.x.download_cell(0, LO + 2)).max() > 0.0


def test_an_exception_in_a_callback_reaches_the_caller(env):
    torch, capi, host = env
    p = _P1Problem(torch, host, "tet_1el", False)

    def fail(level):
        raise KeyError(f"level {level}")

    fmg = host.Solver.fmg(p.st, p.gmg, LO, HI, post_cycle=fail)
    p.reset()
    with pytest.raises(KeyError, match=f"level {LO}"):
        fmg.solve(p.A, p.x, p.b, HI)


@pytest.mark.parametrize("counts", [[1], [1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
def test_a_cycle_vector_of_the_wrong_length_raises(env, counts):
    torch, capi, host = env
    p = _P1Problem(torch, host, "tet_1el", False)
    with pytest.raises(host.HytegHostError, match="every level"):
        host.Solver.fmg(p.st, p.gmg, LO, HI, cycles_per_level=counts)
    p2 = host.P2Solver(p.st, LO, HI, pre=2, post=2)
    with pytest.raises(host.HytegHostError, match="every level"):
        host.P2Solver.fmg(p.st, p2, LO, HI, cycles_per_level=counts)
    with pytest.raises(host.HytegHostError, match="multigrid"):
        host.Solver.fmg(p.st, host.Solver.cg(p.st, LO, HI), LO, HI)


@pytest.mark.parametrize("mesh", ["tet_1el", "cube_6el"])
@pytest.mark.parametrize("cycles", [1, [5, 5, 2, 1]], ids=["one cycle per level", "cycles per level"])
def test_p2_fmg_is_the_sequence_issued_by_hand(env, mesh, cycles):
    torch, capi, host = env
    lo, hi = 2, 3
    per_level = [cycles] * (hi + 1) if isinstance(cycles, int) else cycles
    out = []
    for by_hand in (True, False):
        st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
        st.set_stream(torch.cuda.current_stream().cuda_stream)
        A = host.P2ConstantLaplaceOperator(st, lo, hi)
        A.compute_inverse_diagonal()
        x, b = host.P2Function(st, "x", lo, hi), host.P2Function(st, "b", lo, hi)
        for level in range(lo, hi + 1):
            b.interpolate(1.0, level, host.Inner)
        gmg = host.P2Solver(st, lo, hi, relax=2.0 / 3.0, pre=2, post=2, cg_max_iter=200, cg_tol=1e-13)
        if by_hand:
            for level in range(lo, hi + 1):
                for _ in range(per_level[level]):
                    gmg.solve(A, x, b, level)
                if level < hi:
                    host.p2_prolongate(x, level, _fmg_flag(host))
        else:
            host.P2Solver.fmg(st, gmg, lo, hi, cycles_per_level=cycles).solve(A, x, b, hi)
        out.append([x.download(level, c) for level in range(lo, hi + 1) for c in range(st.n_local_cells)])
    for (wv, we), (gv, ge) in zip(*out):
        assert np.array_equal(wv, gv) and np.array_equal(we, ge)
    assert max(np.abs(v).max() for v, e in out[1]) > 0.0
