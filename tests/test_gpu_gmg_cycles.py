"""The host layer's GeometricMultigridSolver (hyteg_amd/host/solvers.hpp) iterate by iterate against the global-matrix restatement of
its cycle (tests/gmgutil.py, pinned on the CPU by test_gmg_reference.py): three cycles, after each of them every entry of x on every
macro-cell, and after the first cycle the restricted residuals it leaves in b on the lower levels.  The bound of a case is
gmgutil.tolerance( d ) = 1e-12 + 50 d with d the case's own float64-against-80-bit difference, measured on the restatement alone.

What a convergence rate cannot see shows here: a smoothing step too few, pre and post swapped, a coarse iterate zeroed on the free
points only (the functions carry junk on the lower levels), a second W-cycle visit missing, a flag dropped in residual,
restrictInto or prolongateAndAdd, shared points smoothed with the wrong neighbour values."""
import time

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


def _storage(env, case, batch):
    host, hu, bu = env
    st = bu.outflow_cube() if case.outflow else host.Storage.from_gmsh(hu.MESHES / f"{case.mesh}.msh")
    if batch is not None:
        st.set_batch_max_level(batch)
    return st


def _upload(f, L, st, u, level):
    for i in range(st.n_local_cells):
        f.upload_cell(i, level, np.ascontiguousarray(u[L.glob.gidx[st.local_cell(i)[0]]]))


def _compare(L, st, f, level, want, start, bound, what, free_only=False):
    """every local cell's array against the restated global vector: relative L2 and largest entry error against max |want| within
    `bound` (free_only: over the free points, where the other entries are junk of another size), the entries the solver's flag
    does not select bit for bit against `start`"""
    num = den = worst = 0.0
    for i in range(st.n_local_cells):
        idx = L.glob.gidx[st.local_cell(i)[0]]
        got, free = f.download_cell(i, level), L.free[idx]
        assert np.array_equal(got[~free], start[idx][~free]), f"{what}: an entry outside Inner | NeumannBoundary changed"
        sel = free if free_only else np.ones_like(free)
        num, den = num + float(((got - want[idx])[sel] ** 2).sum()), den + float((want[idx][sel] ** 2).sum())
        worst = max(worst, float(np.abs((got - want[idx])[sel]).max(initial=0.0)))  # a cell may hold no free point of a coarse level
    scale = float(np.abs(want[L.free]).max())
    l2 = np.sqrt(num / den)
    print(f"{what}: relative L2 error {l2:.3e}, largest entry error / max |.| {worst / scale:.3e} (bound {bound:.3e})")
    assert l2 <= bound and worst <= bound * scale, what


def _solver(env, case, st):
    host = env[0]
    kw = dict(pre=case.pre, post=case.post, wcycle=case.wcycle)
    if case.smoother == "chebyshev":
        radii = [gu.case_radii(case)[l] for l in range(case.lo, case.hi + 1)]
        make = host.DivKGradSolver.gmg_chebyshev if case.divkgrad else host.Solver.gmg_chebyshev
        return make(st, case.lo, case.hi, case.order, radii, **kw)
    if case.divkgrad:
        assert case.smoother == "jacobi"
        return host.DivKGradSolver.gmg(st, case.lo, case.hi, smoother=host.JACOBI, relax=case.relax, **kw)
    code = {"jacobi": host.JACOBI, "gs": host.GAUSS_SEIDEL, "sor": host.SOR, "sgs": host.SYMMETRIC_GAUSS_SEIDEL, "ssor": host.SYMMETRIC_SOR}
    return host.Solver.gmg(st, case.lo, case.hi, smoother=code[case.smoother], relax=case.relax, **kw)


def _run(env, case, batch=None, fused=None):
    host, hu, bu = env
    t0 = time.perf_counter()
    h, want = gu.case_hierarchy(case), gu.restated(case)
    t_cpu = time.perf_counter() - t0
    lo, hi = case.lo, case.hi
    xs0, bs0 = gu.case_inputs(case)
    st = _storage(env, case, batch)
    x, b = host.P1Function(st, "x", lo, hi), host.P1Function(st, "b", lo, hi)
    keep = [x, b]
    for l in range(lo, hi + 1):
        _upload(x, h.levels[l], st, xs0[l], l)
        _upload(b, h.levels[l], st, bs0[l], l)
    if case.divkgrad:
        k = host.P1Function(st, "k", lo, hi)
        for l in range(lo, hi + 1):
            _upload(k, h.levels[l], st, h.levels[l].k, l)
        A = host.P1ElementwiseDivKGrad(st, lo, hi, k)
        A.compute_inverse_diagonal_operator_values()
        keep.append(k)
    else:
        A = host.P1ConstantOperator(st, lo, hi)
        A.compute_inverse_diagonal()
    solver = _solver(env, case, st)
    if fused is not None:
        solver.set_fused(fused)
    name, top = gu.case_id(case), h.levels[hi]
    for n in range(gu.CYCLES):
        solver.solve(A, x, b, hi)
        _compare(top, st, x, hi, want.iterates[n], xs0[hi], gu.tolerance(want.d_x), f"{name} x after cycle {n + 1}")
        if n == 0:  # the restricted residuals: after the first cycle, while they are well-conditioned data (gmgutil.run_case)
            for l in range(lo, hi):
                _compare(h.levels[l], st, b, l, want.b_lower[l], bs0[l], gu.tolerance(want.d_b), f"{name} b on level {l}", free_only=True)
    _compare(top, st, b, hi, bs0[hi], bs0[hi], 0.0, f"{name} b on the top level is read-only")
    for l in range(lo, hi):
        L = h.levels[l]
        for i in range(st.n_local_cells):  # the coarse iterate was zeroed on ALL points, and no correction writes a Dirichlet point
            free = L.free[L.glob.gidx[st.local_cell(i)[0]]]
            assert np.all(x.download_cell(i, l)[~free] == 0.0), f"{name}: x on level {l} is not zero on the Dirichlet points"
    for o in (solver, A, *keep, st):
        o.close()
    print(f"{name}: {time.perf_counter() - t0:.2f} s, of which the restatement {t_cpu:.2f} s")


def _tet_variants():
    return [(c, f) for c in gu.TET_CASES for f in ((True, False) if c.smoother == "chebyshev" else (None,))]


@pytest.mark.parametrize("case,fused", _tet_variants(), ids=lambda v: gu.case_id(v) if isinstance(v, gu.GmgCase) else {None: "", True: "fused", False: "composed"}[v])
def test_cycles_on_one_macro_cell(env, case, fused):
    """tet_1el, levels 2-4 (level 2 has one free point): every smoother, V(3,3) and V(1,2) -- unequal counts catch a swap -- and one
    W(1,1) cycle on levels 2-5; the Chebyshev smoother by its fused steps and by the composed sequence"""
    _run(env, case, fused=fused)


@pytest.mark.parametrize("batch", [6, -1], ids=["batched", "per-cell"])
@pytest.mark.parametrize("case", gu.MULTI_CELL_CASES, ids=gu.case_id)
def test_cycles_on_several_macro_cells(env, case, batch):
    """regular_octahedron_8el levels 0-3 and cube_6el levels 1-3 (one free coarse point each), batched launches and per-cell ones"""
    _run(env, case, batch=batch)


@pytest.mark.parametrize("batch", [None, -1], ids=["default", "per-cell"])
@pytest.mark.parametrize("case", gu.OUTFLOW_CASES, ids=gu.case_id)
def test_cycles_with_a_neumann_part(env, case, batch):
    """cube_24el with bcutil's outflow face (flag 2 -> Neumann), levels 2-3: the free points are Inner | NeumannBoundary"""
    h = gu.case_hierarchy(case)
    types = env[2].point_types(h.levels[case.hi].coords)
    assert (types == env[0].NeumannBoundary).sum() > 0 and np.array_equal(h.levels[case.hi].free, types != env[0].DirichletBoundary)
    _run(env, case, batch=batch)


@pytest.mark.parametrize("case", gu.DIVKGRAD_CASES, ids=gu.case_id)
def test_cycles_of_the_variable_coefficient_operator(env, case):
    """DivKGradSolver.gmg / gmg_chebyshev: an operator without residual(), so the cycle takes its apply + assign branch"""
    _run(env, case)
