"""The host layer's MinResSolver (hyteg_amd/host/minres.hpp) against the numpy restatement of its loop on a global matrix
(gmgutil.minres, pinned on the CPU by test_gmg_reference.py: its iterates minimise the residual over the Krylov space): x after
exactly k iterations, k = 1, 2, 3, 5, 8, without a preconditioner and with JacobiPreconditioner( 2 ).  A wrong sign in the
three-term recurrence of the search directions or a missing rotation of the work functions changes the second or third iterate by
O(1); the bound is gmgutil.tolerance( d ), d measured on the restatement alone.

Solver.minres does not expose MinResSolver::getIterations (Solver.iterations is the CG solver's), so no iteration count is compared."""
import numpy as np
import pytest

import gmgutil as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    import bcutil as bu
    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return host, hu, bu


@pytest.mark.parametrize("case", gu.MINRES_CASES, ids=gu.minres_id)
def test_minres_iterate_matches_the_restated_loop(env, case):
    """regular_octahedron_8el and cube_24el with the outflow face (free = Inner | NeumannBoundary), level 2: nonzero Dirichlet data,
    zero right-hand side, a random start on the free points"""
    _check(env, case, 0.0, gu.minres_restated(case))


def test_minres_stops_where_the_restated_loop_stops(env):
    """rel_tol = 1e-3 with room for 50 iterations: the restated loop stops early, and neither its last |eta| / res_start nor the one
    before lies within 1 % of the tolerance, so rounding cannot move the stop; x is then the iterate of that iteration"""
    case, rel_tol = gu.MinresCase("regular_octahedron_8el", 2, False, 50, 0), 1e-3
    x, etas = gu.run_minres(case, rel_tol=rel_tol)
    x_w, etas_w = gu.run_minres(case, gu.LD, rel_tol=rel_tol)
    x0 = gu.minres_inputs(case.mesh, case.level, case.outflow)[0]
    L = gu.global_level(case.mesh, case.level)
    start = float(np.linalg.norm((L.apply(x0))[L.free]))  # identity preconditioner, b = 0: res_start = || A x0 || on the free points
    ratios = [abs(e) / start for e in etas]
    print(f"the restated loop stops after {len(etas)} iterations: |eta| / res_start = {ratios[-2]:.3e}, {ratios[-1]:.3e}")
    assert 2 < len(etas) == len(etas_w) < 50 and ratios[-1] < 0.99 * rel_tol and ratios[-2] > 1.01 * rel_tol
    _check(env, case, rel_tol, gu.MinresRestated(x, etas, gu.rel(x, x_w)))


def _check(env, case, rel_tol, want):
    host, hu, bu = env
    L, level = gu.global_level(case.mesh, case.level, case.outflow), case.level
    x0, b0 = gu.minres_inputs(case.mesh, case.level, case.outflow)
    st = bu.outflow_cube() if case.outflow else host.Storage.from_gmsh(hu.MESHES / f"{case.mesh}.msh")
    A = host.P1ConstantOperator(st, level, level)
    A.compute_inverse_diagonal()  # the Jacobi preconditioner's smooth_jac reads it
    x, b = host.P1Function(st, "x", level, level), host.P1Function(st, "b", level, level)
    cells = [L.glob.gidx[st.local_cell(i)[0]] for i in range(st.n_local_cells)]
    for i, idx in enumerate(cells):
        x.upload_cell(i, level, np.ascontiguousarray(x0[idx]))
        b.upload_cell(i, level, np.ascontiguousarray(b0[idx]))
    solver = host.Solver.minres(st, level, level, max_iter=case.k, rel_tol=rel_tol, jacobi_iterations=case.m)
    solver.solve(A, x, b, level)
    bound = gu.tolerance(want.d_x)
    num = den = worst = 0.0
    for i, idx in enumerate(cells):
        got, free = x.download_cell(i, level), L.free[idx]
        assert np.array_equal(got[~free], x0[idx][~free]), "the Dirichlet values are those of the start, bit for bit"
        num, den = num + float(((got - want.x[idx]) ** 2).sum()), den + float((want.x[idx] ** 2).sum())
        worst = max(worst, float(np.abs(got - want.x[idx]).max()))
    l2, scale = np.sqrt(num / den), float(np.abs(want.x).max())
    moved = gu.rel(want.x[L.free], x0[L.free])
    print(f"{gu.minres_id(case)}: relative L2 error {l2:.3e}, largest entry error / max |x| {worst / scale:.3e} (bound {bound:.3e}); "
          f"the iterations moved x by {moved:.2e}")
    assert moved > 0.1
    assert l2 <= bound and worst <= bound * scale
    for o in (solver, A, x, b, st):
        o.close()
