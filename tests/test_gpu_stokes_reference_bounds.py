"""The reference's two MINRES Stokes tests on cube_24el, composed as their sources compose them, with the reference's own bounds:
tests/hyteg/convergence/P1Stokes3DMinResConvergenceTest.cpp (P1-P1, an inflow profile at z = 0 and the outflow face z = 1: needs
per-primitive boundary flags) and P2P1Stokes3DMinResConvergenceTest.cpp (Taylor-Hood, colliding flow; its outflow block is
disabled in the source, so every boundary primitive is Dirichlet)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    import bcutil as bu
    import hostutil as hu
    from hyteg_amd import capi, host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, po, hu, bu


def test_p1_stokes_minres_with_inflow_and_outflow_meets_the_reference_bound(env):
    """:57-60 levels 2-3, 5 iterations, tolerance 1e-16; :66-107 the outflow flags; :155 w = inflow profile on the Dirichlet points;
    :166-183 MINRES with StokesBlockDiagonalPreconditioner( 2 velocity steps, V(2,2) Gauss-Seidel multigrid, CG coarse solver );
    :200-205 sum of r^2 over Inner, with r = L u under Inner | NeumannBoundary, divided by the global DoFs, < 3.1e-12"""
    torch, host, po, hu, bu = env
    lo, hi = 2, 3
    st = bu.outflow_cube("single")  # primitive by primitive, as the source does it
    L = host.P1P1StokesOperator(st, lo, hi)
    u, f, r = (host.P1StokesFunction(st, n, lo, hi) for n in ("u", "f", "r"))
    for i in range(st.n_local_cells):
        P = hu.cell_points(st.local_cell(i)[1], hi)
        inflow = np.where(P[:, 2] < 1e-8, (1.0 / 16.0) * P[:, 0] * (1 - P[:, 0]) * P[:, 1] * (1.0 - P[:, 1]), 0.0)
        u.w.upload_cell(i, hi, np.where(bu.point_types(P) == host.DirichletBoundary, inflow, 0.0))
    solver = host.StokesSolver.minres(st, lo, hi, max_iter=5, rel_tol=1e-16, preconditioner="block", velocity_steps=2)
    solver.solve(L, u, f, hi)
    L.apply(u, r, hi, host.Inner | host.NeumannBoundary)
    dofs = 4 * st.number_of_dofs(hi)
    residual = r.dot(r, hi, host.Inner) / dofs
    # the outflow face carries flow: the natural condition is in force there
    out = max(np.abs(u.w.download_cell(i, hi)[s]).max() for i, s in enumerate(bu.truth(st, hi, host.NeumannBoundary)) if s.any())
    print(f"P1 Stokes MINRES: residual {residual:.4e} (bound 3.1e-12), {dofs} DoFs, max |w| on the outflow face {out:.3e}")
    assert residual < 3.1e-12
    assert out > 0.0
    for o in (solver, u, f, r, L, st):
        o.close()


def test_taylor_hood_stokes_minres_meets_the_reference_bounds(env):
    """:52-55 level 2, 20 iterations, tolerance 1e-13; :163-165 colliding flow on the Dirichlet points, the exact solution;
    :170-177 MINRES with StokesPressureBlockPreconditioner; :179-195 pressure means projected out, r = L u under
    Inner | NeumannBoundary, discrete L2 norms over all DoFs divided by the global DoFs; :211-213 the three bounds"""
    torch, host, po, hu, bu = env
    level = 2
    st = host.Storage.from_gmsh(bu.CUBE)
    L = host.TaylorHoodStokesOperator(st, level, level)
    u, f, r, exact, err = (host.TaylorHoodFunction(st, n, level, level) for n in ("u", "f", "r", "uExact", "err"))
    flow = [lambda x, y, z: 20.0 * x * y ** 3, lambda x, y, z: 5.0 * x ** 4 - 5.0 * y ** 4, lambda x, y, z: 0.0 * x]
    pressure = lambda x, y, z: 60.0 * x ** 2 * y - 20.0 * y ** 3  # noqa: E731
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        pv, pe = hu.cell_points(co, level), po.edge_midpoints(co, level)
        dv, de = bu.point_types(pv) != host.Inner, bu.point_types(pe) != host.Inner  # every boundary point is Dirichlet here
        for k in range(3):
            v, e = flow[k](pv[:, 0], pv[:, 1], pv[:, 2]), flow[k](pe[:, 0], pe[:, 1], pe[:, 2])
            u.velocity[k].upload(level, np.where(dv, v, 0.0), np.where(de, e, 0.0), cell=i)
            exact.velocity[k].upload(level, v, e, cell=i)
        exact.pressure.upload_cell(i, level, pressure(pv[:, 0], pv[:, 1], pv[:, 2]))
    solver = host.TaylorHoodSolver.minres(st, level, level, max_iter=20, rel_tol=1e-13)
    solver.solve(L, u, f, level)
    u.project_pressure_mean(level)
    exact.project_pressure_mean(level)
    L.apply(u, r, level, host.Inner | host.NeumannBoundary)
    err.assign([1.0, -1.0], [u, exact], level)
    dofs = 3 * st.number_of_dofs(level, p2=True) + st.number_of_dofs(level)
    e_uvw = [np.sqrt(err.velocity[k].dot(err.velocity[k], level) / dofs) for k in range(3)]
    e_p = np.sqrt(err.pressure.dot(err.pressure, level) / dofs)
    res = np.sqrt(r.dot(r, level) / dofs)
    print(f"Taylor-Hood MINRES: errors u {e_uvw[0]:.4e} v {e_uvw[1]:.4e} w {e_uvw[2]:.4e} (sum {sum(e_uvw):.4e}, bound 0.6417), "
          f"p {e_p:.4e} (bound 4.003), residual {res:.4e} (bound 0.01934), {dofs} DoFs")
    assert sum(e_uvw) < 0.6417
    assert e_p < 4.003
    assert res < 0.01934
    for o in (solver, u, f, r, exact, err, L, st):
        o.close()
