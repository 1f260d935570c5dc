"""StrongFreeSlipWrapper and MINRES on a wrapped P1-P1 Stokes operator: the wrapper against the composition of the existing
operator and the numpy projection, its symmetry and the vanishing normal component, and the channel with a symmetry plane of
tests/hyteg/freeslip/FreeslipRectangularChannelTest.cpp in 3-D, where free slip on the plane y = 0 is the same discrete problem
as "v Dirichlet, u and w Neumann" -- which the plain operator and the plain MINRES already solve."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from freesliputil import CENTRE, make_storage, radial_about  # noqa: E402


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host


def _fill(f, level, seed):
    import freesliputil as fu

    return [fu.fill_random(f.components[k], level, seed + k) for k in range(4)]


def _download(f, level):
    import hostutil as hu

    return [hu.download(f.components[k], level) for k in range(4)]


def _upload(f, arrays, level):
    import hostutil as hu

    for k in range(4):
        hu.upload(f.components[k], arrays[k], level)


def _project(st, level, arrays, normals, selected):
    import freesliputil as fu

    out = [[], [], [], [a.copy() for a in arrays[3]]]
    for c in range(st.n_local_cells):
        for k, a in enumerate(fu.project_numpy(arrays[0][c], arrays[1][c], arrays[2][c], normals[c], selected[c])):
            out[k].append(a)
    return out


def _setup(host, mesh, level, pre):
    import freesliputil as fu
    import hostutil as hu

    st = make_storage(host, mesh)
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)
    normal = radial_about((0.0, 0.0, 0.0) if mesh == "shell60" else CENTRE)
    op = host.P1P1StokesOperator(st, level, level)
    proj = host.P1ProjectNormalOperator(st, level, level, normal)
    W = host.StrongFreeSlipWrapper(op, proj, host.FreeslipBoundary, pre_projection=pre)
    selected = fu.selected_points(st, level, host.FreeslipBoundary)
    normals = []
    for c in range(st.n_local_cells):
        p = hu.cell_points(st.local_cell(c)[1], level)
        n = np.zeros((len(p), 3))
        n[selected[c]] = np.array([normal(*q) for q in p[selected[c]]], dtype=np.float64).reshape(-1, 3)
        normals.append(n)
    return st, op, proj, W, selected, normals


FLAG = 1 | 4 | 8  # Inner | NeumannBoundary | FreeslipBoundary: what MINRES iterates on


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("mesh,level", [("shell60", 2), ("cube_6el", 3)])
def test_wrapper_is_the_operator_between_projections(env, mesh, level, pre):
    torch, capi, host = env
    import freesliputil as fu

    st, op, proj, W, selected, normals = _setup(host, mesh, level, pre)
    x, y, t = (host.P1StokesFunction(st, n, level, level) for n in ("x", "y", "t"))
    xh = _fill(x, level, 100)
    W.apply(x, y, level, FLAG)
    got = _download(y, level)
    assert all(np.array_equal(a, b) for k in range(4) for a, b in zip(_download(x, level)[k], xh[k])), "apply changed its source"
    # the same from the parts: numpy projection of the source (pre-projection), the existing operator, numpy projection
    _upload(t, _project(st, level, xh, normals, selected) if pre else xh, level)
    ref = host.P1StokesFunction(st, "ref", level, level)
    op.apply(t, ref, level, FLAG)
    want = _project(st, level, _download(ref, level), normals, selected)
    for k in range(4):
        err = fu.rel_l2(got[k], want[k])
        print(f"{mesh} level {level} pre_projection {pre} component {k}: relative L2 error {err:.3e}")
        assert err <= 1e-13
    # ( W x ) . n vanishes at every free-slip point
    top = max(np.abs(np.concatenate(got[k])).max() for k in range(3))
    worst = 0.0
    for c in range(st.n_local_cells):
        s = selected[c]
        dn = sum(got[k][c][s] * normals[c][s, k] for k in range(3))
        worst = max(worst, np.abs(dn).max())
    print(f"largest normal component {worst:.3e}, largest velocity entry {top:.3e}")
    assert worst <= 1e-14 * top


@pytest.mark.parametrize("mesh,level", [("shell60", 2), ("cube_6el", 3)])
def test_wrapper_with_pre_projection_is_symmetric(env, mesh, level):
    torch, capi, host = env
    st, op, proj, W, selected, normals = _setup(host, mesh, level, True)
    x, y, wx, wy = (host.P1StokesFunction(st, n, level, level) for n in ("x", "y", "wx", "wy"))
    _fill(x, level, 200)
    _fill(y, level, 300)
    W.apply(x, wx, level, FLAG)
    W.apply(y, wy, level, FLAG)
    a, b = y.dot(wx, level, host.All), x.dot(wy, level, host.All)
    print(f"<y, W x> = {a!r}, <x, W y> = {b!r}")
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def test_wrapper_with_flag_none_is_the_operator(env):
    torch, capi, host = env
    level = 2
    st = make_storage(host, "cube_6el")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)
    op = host.P1P1StokesOperator(st, level, level)
    proj = host.P1ProjectNormalOperator(st, level, level, radial_about(CENTRE))
    x, y, ref = (host.P1StokesFunction(st, n, level, level) for n in ("x", "y", "ref"))
    _fill(x, level, 5)
    op.apply(x, ref, level, FLAG)
    for pre in (False, True):
        W = host.StrongFreeSlipWrapper(op, proj, 0, pre_projection=pre)
        W.apply(x, y, level, FLAG)
        assert all(np.array_equal(a, b) for k in range(4) for a, b in zip(_download(y, level)[k], _download(ref, level)[k]))


def test_block_preconditioner_is_refused_for_a_wrapped_operator(env):
    torch, capi, host = env
    st = make_storage(host, "tet_1el")
    with pytest.raises(host.HytegHostError, match="block"):
        host.StokesSolver.minres(st, 2, 2, preconditioner="block", free_slip=True)
    plain = host.StokesSolver.minres(st, 2, 2, free_slip=True)
    op = host.P1P1StokesOperator(st, 2, 2)
    f = host.P1StokesFunction(st, "f", 2, 2)
    with pytest.raises(TypeError, match="StrongFreeSlipWrapper"):
        plain.solve(op, f, f, 2)


# ---- the channel: free slip on y = 0 against "v Dirichlet, u and w Neumann" there ----------------------------------------------
EPS = 1e-12


def channel_storage(host):
    """cube_6el flagged in the order of FreeslipRectangularChannelTest.cpp:64-72: outflow x = 1 (2), free slip y = 0 (3), then no
    slip (1) on y = 1, x = 0, z = 0, z = 1, so that the rims towards the no-slip faces end no-slip"""
    import hostutil as hu

    st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
    st.set_mesh_boundary_flags_by_vertex_location(2, lambda x, y, z: abs(x - 1.0) < EPS)
    st.set_mesh_boundary_flags_by_vertex_location(3, lambda x, y, z: abs(y) < EPS)
    for pred in (lambda x, y, z: abs(y - 1.0) < EPS, lambda x, y, z: abs(x) < EPS, lambda x, y, z: abs(z) < EPS,
                 lambda x, y, z: abs(z - 1.0) < EPS):
        st.set_mesh_boundary_flags_by_vertex_location(1, pred)
    return st


def channel_conditions(host):
    """problem A: flag 3 is Neumann for u and w, Dirichlet for v; problem B: flag 3 is free slip for all three"""
    uw = host.BoundaryCondition()
    uw.create_dirichlet("noslip", [1])
    uw.create_neumann("open", [2, 3])
    v = host.BoundaryCondition()
    v.create_dirichlet("noslip", [1, 3])
    v.create_neumann("open", [2])
    return (uw, v, uw), host.BoundaryCondition.create_0123()


class Discretisation:
    """what the channel test needs of P1-P1 ("p1") and Taylor-Hood ("th"): functions as per-cell host arrays (vertex DoFs, and edge DoFs
    for P2), the operator, the projection and the two MINRES solvers"""

    def __init__(self, host, kind):
        self.host, self.kind, self.p2 = host, kind, kind == "th"

    def function(self, st, name, level):
        return (self.host.TaylorHoodFunction if self.p2 else self.host.P1StokesFunction)(st, name, level, level)

    def velocity(self, f):
        return f.velocity if self.p2 else f.uvw

    def pressure(self, f):
        return f.pressure if self.p2 else f.p

    def operator(self, st, level):
        return (self.host.TaylorHoodStokesOperator if self.p2 else self.host.P1P1StokesOperator)(st, level, level)

    def projection(self, st, level, normal):
        return (self.host.P2ProjectNormalOperator if self.p2 else self.host.P1ProjectNormalOperator)(st, level, level, normal)

    def minres(self, st, level, **kw):
        return (self.host.TaylorHoodSolver if self.p2 else self.host.StokesSolver).minres(st, level, level, **kw)

    def points(self, st, c, level):
        """coordinates of the DoFs of a velocity component in cell c: vertex DoFs, then (P2) edge DoFs, rounded so that the copies of a
        shared DoF get the same bits"""
        import freesliputil as fu
        import hostutil as hu

        co = st.local_cell(c)[1]
        p = hu.cell_points(co, level)
        return np.round(np.vstack([p, fu.edge_points(co, level)]) if self.p2 else p, 12)

    def selected(self, st, c, level, flag, bc):
        import freesliputil as fu
        import hostutil as hu

        m = st.mask(c, flag, bc=bc)
        v = hu.point_mask(level, m)
        return np.concatenate([v, fu.edge_mask(level, m)]) if self.p2 else v

    def get(self, f, c, level):
        if self.p2:
            return np.concatenate(f.download(level, cell=c))
        return f.download_cell(c, level)

    def put(self, f, c, level, values):
        if self.p2:
            nv = f.sizes(level)[0]
            f.upload(level, values[:nv], values[nv:], cell=c)
        else:
            f.upload_cell(c, level, values)


def exact_u(p):
    return (1.0 - p[:, 1]) * (1.0 + p[:, 1])


def dirichlet_data(D, st, f, level):
    """u = ( ( 1 - y )( 1 + y ), 0, 0 ) on the Dirichlet points of every component, zero elsewhere"""
    f.interpolate(0.0, level, D.host.All) if D.p2 else [g.interpolate(0.0, level, D.host.All) for g in f.components]
    u = D.velocity(f)[0]
    for c in range(st.n_local_cells):
        on = D.selected(st, c, level, D.host.DirichletBoundary, u.boundary_condition)
        D.put(u, c, level, np.where(on, exact_u(D.points(st, c, level)), 0.0))


def with_conditions(D, st, name, level, bcs):
    f = D.function(st, name, level)
    if isinstance(bcs, tuple):
        for k in range(3):
            f.set_velocity_boundary_condition(bcs[k], k)
    else:
        f.set_velocity_boundary_condition(bcs)
    return f


def residual_norm(D, st, op, x, level, bcs):
    """|| f - A x || with f = 0 over the unknowns of problem A"""
    r = with_conditions(D, st, "r", level, bcs)
    op.apply(x, r, level, FLAG)
    return np.sqrt(r.dot(r, level, FLAG))


def error_norm(D, st, x, level):
    """the norm of the reference's test (lines 141-145): velocity minus the exact one over all DoFs, the pressure left out"""
    total = 0.0
    owned = set()
    for c in range(st.n_local_cells):
        pts = D.points(st, c, level)
        for k in range(3):
            diff = D.get(D.velocity(x)[k], c, level) - (exact_u(pts) if k == 0 else 0.0)
            for i, q in enumerate(pts):  # every DoF once
                key = (k,) + tuple(q)
                if key not in owned:
                    owned.add(key)
                    total += diff[i] ** 2
    return np.sqrt(total)


_solved = {}


def solve_channel(host, kind, level, rel_tol, max_iter):
    """solved once per discretisation and shared by the tests (they only read the result)"""
    key = (kind, level, rel_tol, max_iter)
    if key not in _solved:
        _solved[key] = _solve_channel(host, kind, level, rel_tol, max_iter)
    return _solved[key]


def _solve_channel(host, kind, level, rel_tol, max_iter):
    D = Discretisation(host, kind)
    st = channel_storage(host)
    bcA, bcB = channel_conditions(host)
    op = D.operator(st, level)
    xA, bA = with_conditions(D, st, "xA", level, bcA), with_conditions(D, st, "bA", level, bcA)
    xB, bB = with_conditions(D, st, "xB", level, bcB), with_conditions(D, st, "bB", level, bcB)
    dirichlet_data(D, st, xA, level)
    dirichlet_data(D, st, xB, level)
    for c in range(st.n_local_cells):
        for k in range(3):
            assert np.array_equal(D.get(D.velocity(xA)[k], c, level), D.get(D.velocity(xB)[k], c, level))
    solverA = D.minres(st, level, max_iter=max_iter, rel_tol=rel_tol)
    solverA.solve(op, xA, bA, level)
    proj = D.projection(st, level, lambda x, y, z: (0.0, -1.0, 0.0))
    W = host.StrongFreeSlipWrapper(op, proj, host.FreeslipBoundary)
    solverB = D.minres(st, level, max_iter=max_iter, rel_tol=rel_tol, free_slip=True)
    solverB.solve(W, xB, bB, level)
    # B's solution judged by A's operator: its values in a function with A's conditions
    xBA = with_conditions(D, st, "xBA", level, bcA)
    for c in range(st.n_local_cells):
        for k in range(3):
            D.put(D.velocity(xBA)[k], c, level, D.get(D.velocity(xB)[k], c, level))
        D.pressure(xBA).upload_cell(c, level, D.pressure(xB).download_cell(c, level))
    rA, rB = residual_norm(D, st, op, xA, level, bcA), residual_norm(D, st, op, xBA, level, bcA)
    return D, st, xA, xB, rA, rB, bcB


@pytest.mark.parametrize("kind", ["p1", "th"])
def test_free_slip_channel_is_the_same_problem_as_mixed_conditions(env, kind):
    """cube_6el, level 2, rel_tol 1e-10 and at most 1000 iterations for both problems.  Measured on an MI355X:
    P1-P1: residual of A's own solution 9.733309e-11, of B's solution under A's operator 9.733309e-11; Taylor-Hood: 1.750849e-10 and
    1.750849e-10."""
    torch, capi, host = env
    level = 2
    D, st, xA, xB, rA, rB, bcB = solve_channel(host, kind, level, 1e-10, 1000)
    print(f"{kind} channel: residual of A's solution {rA:.6e}, of B's solution under A's operator {rB:.6e}")
    assert np.isfinite(rA) and np.isfinite(rB)
    assert rB <= 10.0 * rA
    # v on the symmetry plane is exactly zero, and the plane has free-slip DoFs
    count = 0
    v = D.velocity(xB)[1]
    for c in range(st.n_local_cells):
        on = D.selected(st, c, level, host.FreeslipBoundary, bcB)
        count += int(on.sum())
        assert (D.get(v, c, level)[on] == 0.0).all()
    assert count > 0
    # and the flow is not trivial
    assert max(np.abs(D.get(D.velocity(xB)[0], c, level)).max() for c in range(st.n_local_cells)) > 0.5


def test_taylor_hood_free_slip_channel_reaches_the_exact_quadratic_velocity(env):
    """u = ( ( 1 - y )( 1 + y ), 0, 0 ), p = 2 ( 1 - x ) solves the channel exactly and lies in the Taylor-Hood space: the error
    of the free-slip solve (B) against the error the mixed-condition solve (A) reaches with the same tolerance and iteration limit.
    Measured on an MI355X: 1.529266e-09 for A and 1.529266e-09 for B."""
    torch, capi, host = env
    level = 2
    D, st, xA, xB, rA, rB, bcB = solve_channel(host, "th", level, 1e-10, 1000)
    eA, eB = error_norm(D, st, xA, level), error_norm(D, st, xB, level)
    print(f"Taylor-Hood channel: velocity error of A {eA:.6e}, of B {eB:.6e}")
    assert np.isfinite(eA) and np.isfinite(eB)
    assert eB <= 10.0 * eA
