"""Per-primitive boundary conditions on the GPU: the host layer's operators, smoothers, vector kernels, reductions, grid
transfer and solvers on storages whose boundary has a Dirichlet and a Neumann part.  What is selected is decided in the tests
from coordinates alone (bcutil.point_types); values are compared with the global-matrix restatement of hostutil and with the
single-cell CPU oracle."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
IN = 1 | 4  # host.Inner | host.NeumannBoundary


@pytest.fixture(scope="module")
def env():
    import torch

    import bcutil as bu
    import chebyshevutil as cu
    import hostutil as hu
    from hyteg_amd import capi, host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, po, hu, bu, cu


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


_globals = {}


def _glob(hu, mesh, level):
    """the global matrix of a mesh and level, built once and left unchanged"""
    if (mesh, level) not in _globals:
        v, c = hu.read_msh(hu.MESHES / f"{mesh}.msh")
        _globals[(mesh, level)] = hu.GlobalSweepOracle(v, c, level)
    return _globals[(mesh, level)]


# ---- 6. the flags are fixed once a function exists ------------------------------------------------------------------
def test_flag_setters_throw_after_a_function_has_been_created(env):
    torch, host, po, hu, bu, cu = env
    st = host.Storage.from_gmsh(bu.CUBE)
    st.set_mesh_boundary_flag(2, 0, 2)
    f = host.P1Function(st, "f", 2, 2)
    with pytest.raises(host.HytegHostError, match="flags are fixed"):
        st.set_mesh_boundary_flag(2, 0, 1)
    with pytest.raises(host.HytegHostError, match="flags are fixed"):
        st.set_mesh_boundary_flags_by_centroid_location(2, bu.on_outflow)
    f.close()
    st.close()


# ---- 7. apply, entry by entry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("batch", [None, -1])
@pytest.mark.parametrize("kind", ["constant", "elementwise"])
def test_apply_on_the_outflow_cube_matches_the_global_matrix(env, level, batch, kind):
    torch, host, po, hu, bu, cu = env
    glob = _glob(hu, "cube_24el", level)
    st = bu.outflow_cube()
    if batch is not None:
        st.set_batch_max_level(batch)
    A = host.P1ConstantOperator(st, level, level) if kind == "constant" else host.P1ElementwiseDiffusion(st, level, level)
    rng = np.random.default_rng(10 + level)
    u, prior = rng.standard_normal(glob.ndof), rng.standard_normal(glob.ndof) + 3.0
    want = glob.matvec(u)
    src, dst = host.P1Function(st, "src", level, level), host.P1Function(st, "dst", level, level)
    hu.upload(src, glob.to_cells(u), level)
    for flag in (host.Inner | host.NeumannBoundary, host.NeumannBoundary):
        hu.upload(dst, glob.to_cells(prior), level)
        A.apply(src, dst, level, flag)
        got = hu.download(dst, level)
        sel = bu.truth(st, level, flag)
        assert sum(int(s.sum()) for s in sel) > 0
        a = np.concatenate([g[s] for g, s in zip(got, sel)])
        w = np.concatenate([want[gi][s] for gi, s in zip(glob.gidx, sel)])
        err = _rel(a, w)
        print(f"{kind} level {level} batch {batch} flag {flag}: relative L2 error {err:.3e}")
        assert err <= 1e-12
        for g, gi, s in zip(got, glob.gidx, sel):
            assert np.array_equal(g[~s], prior[gi][~s]), "points the flag does not select keep their contents"
    for o in (src, dst, A, st):
        o.close()


# ---- 8. one cell, one Neumann face ----------------------------------------------------------------------------------
def _one_cell(host, tet):
    st = host.Storage.single_tet(tet)
    face = [i for i in range(st.n_faces) if st.primitive(2, i).vertex_ids == (0, 1, 2)]
    assert len(face) == 1
    st.set_mesh_boundary_flag(2, face[0], 2)
    return st


@pytest.mark.parametrize("level", [2, 4])
def test_one_cell_with_a_neumann_face(env, level):
    from conftest import SKEW_TET

    torch, host, po, hu, bu, cu = env
    st = _one_cell(host, SKEW_TET)
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    flag = host.Inner | host.NeumannBoundary
    mask = st.mask(0, flag)
    assert mask == po.MASK_INNER | (1 << 6)  # the interior and face 0 = (0, 1, 2); its edges and vertices stay Dirichlet
    m = hu.point_mask(level, mask)
    orc = hu.MultiCellOracle(st)
    n = po.cell_size(level)
    rng = np.random.default_rng(20 + level)
    A = host.P1ConstantOperator(st, level, level)
    A.compute_inverse_diagonal()
    inv = hu.download(A.inverse_diagonal(level, level), level)
    fs = [host.P1Function(st, f"f{k}", level, level) for k in range(8)]

    # apply
    u, prior = rng.standard_normal(n), rng.standard_normal(n)
    hu.upload(fs[0], [u], level)
    hu.upload(fs[1], [prior], level)
    A.apply(fs[0], fs[1], level, flag)
    want = orc.apply([u], [prior.copy()], level, flag)[0]
    got = fs[1].download_cell(0, level)
    assert _rel(got[m], want[m]) <= 1e-12 and np.array_equal(got[~m], prior[~m])
    assert not np.array_equal(got[hu.point_mask(level, 1 << 6)], prior[hu.point_mask(level, 1 << 6)])  # the face was written

    # apply_cycle over 4 pairs: shell points are selected, so the steps launch is not taken
    us = [rng.standard_normal(n) for _ in range(4)]
    for k in range(4):
        hu.upload(fs[k], [us[k]], level)
        hu.upload(fs[4 + k], [prior], level)
    A.apply_cycle(fs[:4], fs[4:], level, flag, host.Replace, 0, 4)
    assert st.steps_launches() == 0
    A.apply_cycle(fs[:4], fs[4:], level, host.Inner, host.Replace, 0, 4)  # the counter-check: the interior alone is grouped
    assert st.steps_launches() > 0
    for k in range(4):
        hu.upload(fs[4 + k], [prior], level)
    A.apply_cycle(fs[:4], fs[4:], level, flag, host.Replace, 0, 4)
    for k in range(4):
        want = orc.apply([us[k]], [prior.copy()], level, flag)[0]
        got = fs[4 + k].download_cell(0, level)
        assert _rel(got[m], want[m]) <= 1e-12 and np.array_equal(got[~m], prior[~m])

    # smooth_jac: dst = src + relax D^-1 ( rhs - A src ) on the selected points
    src, rhs, relax = rng.standard_normal(n), rng.standard_normal(n), 0.7
    hu.upload(fs[0], [src], level)
    hu.upload(fs[1], [rhs], level)
    hu.upload(fs[2], [prior], level)
    A.smooth_jac(fs[2], fs[1], fs[0], relax, level, flag)
    asrc = orc.apply([src], [np.zeros(n)], level, flag)[0]
    want = src + relax * inv[0] * (rhs - asrc)
    got = fs[2].download_cell(0, level)
    assert _rel(got[m], want[m]) <= 1e-12 and np.array_equal(got[~m], prior[~m])

    # the Chebyshev(3) smoother, fused where it may be and composed
    rho = 1.9
    c = cu.coefficients(3, 0.3 * rho, 1.2 * rho)
    want = cu.multi_cell_smooth(orc, st, [src], [rhs], inv, c, level, flag, hu.point_mask)[0]
    sm = host.Solver.chebyshev(st, level, level, 3, rho)
    for fused in (True, False):
        sm.set_fused(fused)
        hu.upload(fs[0], [src], level)
        sm.solve(A, fs[0], fs[1], level)
        got = fs[0].download_cell(0, level)
        assert _rel(got, want) <= 1e-12 and np.array_equal(got[~m], src[~m])
        assert not np.array_equal(got[hu.point_mask(level, 1 << 6)], src[hu.point_mask(level, 1 << 6)])
    for o in (sm, *fs, A, st):
        o.close()


F32_TOL = 2e-6  # relative error of an increment formed by the float kernels: the bar of tests/test_gpu_fp32.py


@pytest.mark.parametrize("level", [2, 4])
@pytest.mark.parametrize("fp32_sweeps", [2, 3])
def test_mixed_precision_jacobi_steps_with_a_neumann_face_match_the_composition(env, level, fp32_sweeps):
    """MixedPrecisionJacobiSmoother::solveSteps( n ) may run n float sweeps on the cell interior alone only while no shell point
    is selected.  With a Neumann face each step is: fp32Sweeps float Jacobi sweeps on the error equation A e = b - A x over the
    interior with e = 0 on the shell, x += e, then one double smooth_jac over mask = INNER | 1 << 6.  The composition is built
    here from the oracle's single-cell functions in double.  What the float kernels add is a relative error of F32_TOL in the
    increment of a step (the bar of the existing float tests); a Jacobi step with relax 0.7 does not amplify differences, so the
    increment of n steps agrees within n * F32_TOL; the double part alone would agree to 1e-12."""
    from conftest import SKEW_TET

    torch, host, po, hu, bu, cu = env
    steps, relax, flag = 3, 0.7, host.Inner | host.NeumannBoundary
    st = _one_cell(host, SKEW_TET)
    mask = st.mask(0, flag)
    assert mask == po.MASK_INNER | (1 << 6)
    m, face, inner = hu.point_mask(level, mask), hu.point_mask(level, 1 << 6), hu.point_mask(level, po.MASK_INNER)
    orc = hu.MultiCellOracle(st)
    A = host.P1ConstantOperator(st, level, level)
    A.compute_inverse_diagonal()
    inv = hu.download(A.inverse_diagonal(level, level), level)[0]
    w = po.assemble_cell_stencil(st.local_cell(0)[1], level)
    n = po.cell_size(level)
    rng = np.random.default_rng(50 + level)
    x0, b0 = rng.standard_normal(n), rng.standard_normal(n)

    def interior_apply(v):
        out = np.zeros(n)
        po.apply_cell(out, v, level, w)
        return np.where(inner, out, 0.0)

    want = x0.copy()
    for _ in range(steps):
        r = np.where(inner, b0 - interior_apply(want), 0.0)
        e = relax * r / w[7]
        for _ in range(fp32_sweeps - 1):
            e = e + relax * (r - interior_apply(e)) / w[7]  # e stays zero on the shell
        want = want + e
        ax = orc.apply([want], [np.zeros(n)], level, flag)[0]
        want = np.where(m, want + relax * inv * (b0 - ax), want)
    x, b = host.P1Function(st, "x", level, level), host.P1Function(st, "b", level, level)
    hu.upload(x, [x0], level)
    hu.upload(b, [b0], level)
    sm = host.Solver.mixed_precision_jacobi(st, level, level, relax=relax, fp32_sweeps=fp32_sweeps)
    sm.solve_steps(A, x, b, level, steps)
    got = x.download_cell(0, level)
    err = _rel((got - x0)[m], (want - x0)[m])
    print(f"level {level}, {fp32_sweeps} float sweeps: relative error of the increment {err:.3e}, on the face {_rel((got - x0)[face], (want - x0)[face]):.3e}")
    assert err <= steps * F32_TOL
    assert _rel((got - x0)[face], (want - x0)[face]) <= steps * F32_TOL
    assert np.all(got[face] != x0[face]), "the face points are swept"
    assert np.array_equal(got[~m], x0[~m]), "points the flag does not select keep their bits"
    for o in (sm, x, b, A, st):
        o.close()


# ---- 9. Gauss-Seidel / SOR in the reference's order -----------------------------------------------------------------
@pytest.mark.parametrize("relax,backwards", [(1.0, False), (1.3, False), (1.3, True)])
@pytest.mark.parametrize("batch", [None, -1])
def test_sweeps_with_a_neumann_part_match_the_reference_order(env, relax, backwards, batch):
    torch, host, po, hu, bu, cu = env
    level, mesh = 2, "cube_6el"
    glob = _glob(hu, mesh, level)
    st = bu.outflow_cube(mesh=hu.MESHES / f"{mesh}.msh")
    flagged = [(d, i) for d in range(3) for i in range(st.n_primitives(d)) if st.primitive(d, i).flag == 2]
    assert sorted(d for d, _ in flagged) == [1, 2, 2]  # the two faces of z = 1 and the edge between them
    if batch is not None:
        st.set_batch_max_level(batch)
    # "primitive is Dirichlet-typed", per global point, from the coordinates of the point
    coords = np.zeros((glob.ndof, 3))
    for i in range(st.n_local_cells):
        gid, co, _ = st.local_cell(i)
        coords[glob.gidx[gid]] = hu.cell_points(co, level)
    dirichlet = list(bu.point_types(coords) == host.DirichletBoundary)
    A = host.P1ConstantOperator(st, level, level)
    x, rhs = host.P1Function(st, "x", level, level), host.P1Function(st, "b", level, level)
    rng = np.random.default_rng(30)
    u, b = rng.standard_normal(glob.ndof), rng.standard_normal(glob.ndof)
    hu.upload(x, glob.to_cells(u), level)
    hu.upload(rhs, glob.to_cells(b), level)
    if relax == 1.0:
        A.smooth_gs(x, rhs, level, host.Inner | host.NeumannBoundary)
    else:
        A.smooth_sor(x, rhs, relax, level, host.Inner | host.NeumannBoundary, backwards)
    saved, glob.boundary = glob.boundary, dirichlet
    try:
        want = glob.sweep(u, b, relax, backwards)
    finally:
        glob.boundary = saved
    got = hu.download(x, level)
    assert np.any(want[~np.array(dirichlet)] != u[~np.array(dirichlet)])
    for g, a in zip(glob.gidx, got):
        assert np.abs(a - want[g]).max() <= 1e-12 * np.abs(want).max()  # the bar of test_gpu_sor_shell.py
    ref = glob.to_global(got)
    for g, a in zip(glob.gidx, got):
        assert np.array_equal(a, ref[g])  # all copies of a shared DoF carry the same bits
    for o in (x, rhs, A, st):
        o.close()


# ---- 10. vector kernels, dot, reductions, transfer ------------------------------------------------------------------
def test_vector_kernels_and_reductions_on_the_outflow_cube(env):
    torch, host, po, hu, bu, cu = env
    level = 2
    glob = _glob(hu, "cube_24el", level)
    st = bu.outflow_cube()
    coords = np.zeros((glob.ndof, 3))
    for i in range(st.n_local_cells):
        coords[glob.gidx[st.local_cell(i)[0]]] = hu.cell_points(st.local_cell(i)[1], level)
    types = bu.point_types(coords)  # every physical point once
    rng = np.random.default_rng(40)
    a, b = rng.standard_normal(glob.ndof), rng.standard_normal(glob.ndof)
    f, g = host.P1Function(st, "f", level, level), host.P1Function(st, "g", level, level)

    def cells(u):
        return [u[glob.gidx[st.local_cell(i)[0]]] for i in range(st.n_local_cells)]

    for flag in (host.Inner | host.NeumannBoundary, host.NeumannBoundary, host.DirichletBoundary):
        sel = (types & flag) != 0
        hu.upload(f, cells(a), level)
        hu.upload(g, cells(b), level)
        f.assign([2.0, -0.5], [f, g], level, flag)
        want = np.where(sel, 2.0 * a - 0.5 * b, a)
        for got, w in zip(hu.download(f, level), cells(want)):
            assert np.array_equal(got, w)
        hu.upload(f, cells(a), level)
        assert abs(f.dot(g, level, flag) - float(a[sel] @ b[sel])) <= 1e-12 * float(np.abs(a[sel]) @ np.abs(b[sel]))
        assert abs(f.sum(level, flag) - a[sel].sum()) <= 1e-12 * np.abs(a[sel]).sum()
        # the extrema always include the cell interiors (the reference's rule): interior of a macro-cell = not on any macro-face
        slot = po.slot_of_points(level)
        interior = np.zeros(glob.ndof, dtype=bool)
        for i in range(st.n_local_cells):
            interior[glob.gidx[st.local_cell(i)[0]][slot == 14]] = True
        assert f.max_magnitude(level, flag) == np.abs(a[sel | interior]).max()
        f.interpolate(7.5, level, flag)
        for got, w in zip(hu.download(f, level), cells(np.where(sel, 7.5, a))):
            assert np.array_equal(got, w)
    # interpolate on one boundary of the function's condition: the uid of flag 2
    bc = f.boundary_condition
    assert bc == host.BoundaryCondition.create_0123()
    hu.upload(f, cells(a), level)
    f.interpolate(-3.0, level, boundary_uid=bc.boundary_uid(2))
    for got, w in zip(hu.download(f, level), cells(np.where(types == host.NeumannBoundary, -3.0, a))):
        assert np.array_equal(got, w)
    f.interpolate(4.0, level, boundary_uid=bc.boundary_uid(0))  # the flags without a boundary: the interior
    for got, w in zip(hu.download(f, level), cells(np.where(types == host.NeumannBoundary, -3.0, np.where(types == host.Inner, 4.0, a)))):
        assert np.array_equal(got, w)
    # a function with a condition of its own reads the same flags differently
    own = host.BoundaryCondition()
    lid = own.create_dirichlet("lid", 2)
    own.create_neumann("free", [1])
    g.set_boundary_condition(own)
    assert g.boundary_condition == own and g.boundary_condition != bc
    hu.upload(g, cells(b), level)
    g.interpolate(1.25, level, host.DirichletBoundary)
    for got, w in zip(hu.download(g, level), cells(np.where(types == host.NeumannBoundary, 1.25, b))):
        assert np.array_equal(got, w)
    g.interpolate(2.5, level, boundary_uid=lid)
    for got, w in zip(hu.download(g, level), cells(np.where(types == host.NeumannBoundary, 2.5, b))):
        assert np.array_equal(got, w)
    g.set_all_inner()
    assert g.boundary_condition == host.BoundaryCondition.create_all_inner()
    g.interpolate(9.0, level, host.Inner)
    for got in hu.download(g, level):
        assert np.all(got == 9.0)
    for o in (f, g, st):
        o.close()


@pytest.mark.parametrize("batch", [None, -1])
def test_grid_transfer_under_inner_and_neumann(env, batch):
    """restrict 3 -> 2 and prolongate 2 -> 3 under Inner | NeumannBoundary give, on the points the coordinates select, what the
    same call gives under All (the path the existing transfer tests pin down), and leave every other point alone"""
    torch, host, po, hu, bu, cu = env
    st = bu.outflow_cube()
    if batch is not None:
        st.set_batch_max_level(batch)
    orc = hu.MultiCellOracle(st)
    fn = lambda x, y, z: np.sin(3 * x + y) + z * z - 0.3 * x * y  # noqa: E731
    fine, coarse = orc.interpolate(fn, 3), orc.interpolate(lambda x, y, z: np.cos(2 * x - z) + y, 2)
    f, g = host.P1Function(st, "f", 2, 3), host.P1Function(st, "g", 2, 3)
    flag = host.Inner | host.NeumannBoundary
    for h in (f, g):
        hu.upload(h, fine, 3)
        hu.upload(h, coarse, 2)
    host.restrict(f, 3, flag)
    host.restrict(g, 3, host.All)
    for got, full, old, sel in zip(hu.download(f, 2), hu.download(g, 2), coarse, bu.truth(st, 2, flag)):
        assert np.array_equal(got[sel], full[sel]) and np.array_equal(got[~sel], old[~sel])
        assert not np.array_equal(full[~sel], old[~sel])
    for h in (f, g):
        hu.upload(h, coarse, 2)
    host.prolongate(f, 2, flag)
    host.prolongate(g, 2, host.All)
    for got, full, old, sel in zip(hu.download(f, 3), hu.download(g, 3), fine, bu.truth(st, 3, flag)):
        assert np.array_equal(got[sel], full[sel]) and np.array_equal(got[~sel], old[~sel])
    hu.upload(f, fine, 3)
    host.prolongate_and_add(f, 2, flag)  # g still holds the prolongated coarse function on every point
    for got, full, old, sel in zip(hu.download(f, 3), hu.download(g, 3), fine, bu.truth(st, 3, flag)):
        assert np.abs(got[sel] - (old[sel] + full[sel])).max() <= 1e-14 * np.abs(full).max() and np.array_equal(got[~sel], old[~sel])
    for o in (f, g, st):
        o.close()


def _global_types(hu, bu, st, glob, level):
    coords = np.zeros((glob.ndof, 3))
    for i in range(st.n_local_cells):
        coords[glob.gidx[st.local_cell(i)[0]]] = hu.cell_points(st.local_cell(i)[1], level)
    return coords, bu.point_types(coords)


@pytest.mark.parametrize("batch", [None, -1])
def test_prolongation_reproduces_linears_on_the_points_the_coordinates_select(env, batch):
    """the check of test_prolongation_reproduces_linears_across_macro_cells (VertexDoFLinearProlongation3DTest.cpp:46-137, squared
    error < 1e-15 scaled by the data) on the outflow cube under Inner | NeumannBoundary, with the selection from coordinates"""
    torch, host, po, hu, bu, cu = env
    st = bu.outflow_cube()
    if batch is not None:
        st.set_batch_max_level(batch)
    flag = host.Inner | host.NeumannBoundary
    u = host.P1Function(st, "u", 2, 3)
    for fn in (lambda x, y, z: 0 * x + 42.0, lambda x, y, z: 42 * x + y - 7 * z):
        for i in range(st.n_local_cells):
            P = hu.cell_points(st.local_cell(i)[1], 2)
            u.upload_cell(i, 2, fn(P[:, 0], P[:, 1], P[:, 2]))
        u.interpolate(123.0, 3, host.All)
        host.prolongate(u, 2, flag)
        for i, (g, sel) in enumerate(zip(hu.download(u, 3), bu.truth(st, 3, flag))):
            P = hu.cell_points(st.local_cell(i)[1], 3)
            e = fn(P[:, 0], P[:, 1], P[:, 2])
            assert float(((g - e)[sel] ** 2).sum()) < 1e-15 * max(1.0, float((e ** 2).max()))
            assert np.all(g[~sel] == 123.0)
    u.close()
    st.close()


@pytest.mark.parametrize("batch", [None, -1])
def test_restriction_is_the_transpose_of_prolongation_on_the_selected_points(env, batch):
    """< R f, c > over the selected coarse points == < f, P c > over the selected fine points, for f and c that vanish on the
    points the coordinates do not select: R = P^T entry by entry, the 1 / numNeighborCells scaling and the additive exchange of
    the classes 0 and 2 included.  Bound: that of test_restriction_is_the_transpose_of_prolongation_on_the_whole_mesh."""
    torch, host, po, hu, bu, cu = env
    st = bu.outflow_cube()
    if batch is not None:
        st.set_batch_max_level(batch)
    flag = host.Inner | host.NeumannBoundary
    g2, g3 = _glob(hu, "cube_24el", 2), _glob(hu, "cube_24el", 3)
    t2, t3 = _global_types(hu, bu, st, g2, 2)[1], _global_types(hu, bu, st, g3, 3)[1]
    rng = np.random.default_rng(60)
    fv = np.where((t3 & flag) != 0, rng.standard_normal(g3.ndof), 0.0)
    cv = np.where((t2 & flag) != 0, rng.standard_normal(g2.ndof), 0.0)
    f, f0, c = (host.P1Function(st, n, 2, 3) for n in ("f", "f0", "c"))
    hu.upload(f, g3.to_cells(fv), 3)
    hu.upload(f0, g3.to_cells(fv), 3)
    hu.upload(c, g2.to_cells(cv), 2)
    host.restrict(f, 3, flag)
    lhs = f.dot(c, 2, flag)
    host.prolongate(c, 2, flag)
    rhs = f0.dot(c, 3, flag)
    print(f"< R f, c > = {lhs:.15e}, < f, P c > = {rhs:.15e}")
    assert abs(rhs) > 1.0 and abs(lhs - rhs) < 1e-11 * abs(rhs)
    for o in (f, f0, c, st):
        o.close()


# ---- conditions of their own on P2 and on the Stokes functions ------------------------------------------------------
def _lid_condition(host):
    """reads the outflow cube the other way round: the inside of z = 1 (flag 2) a wall, the rest of the surface (flag 1) free"""
    bc = host.BoundaryCondition()
    lid = bc.create_dirichlet("lid", 2)
    bc.create_neumann("free", [1])
    return bc, lid


def test_p2_function_with_a_condition_of_its_own(env):
    torch, host, po, hu, bu, cu = env
    level = 2
    st = bu.outflow_cube()
    own, lid = _lid_condition(host)
    f = host.P2Function(st, "f", level, level)
    assert f.boundary_condition == host.BoundaryCondition.create_0123()
    f.set_boundary_condition(own)
    assert f.boundary_condition == own and f.boundary_condition != host.BoundaryCondition.create_0123()
    types = []
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        types.append(np.concatenate([bu.point_types(hu.cell_points(co, level)), bu.point_types(po.edge_midpoints(co, level))]))

    def values():
        return [np.concatenate(f.download(level, cell=i)) for i in range(st.n_local_cells)]

    f.interpolate(1.0, level, host.All)
    f.interpolate(2.0, level, host.DirichletBoundary)  # under the function's condition: the inside of z = 1
    for v, t in zip(values(), types):
        assert np.array_equal(v, np.where(t == host.NeumannBoundary, 2.0, 1.0))
    f.interpolate(3.0, level, host.Inner | host.NeumannBoundary)  # everything else
    for v, t in zip(values(), types):
        assert np.array_equal(v, np.where(t == host.NeumannBoundary, 2.0, 3.0))
    f.interpolate(4.0, level, boundary_uid=lid)
    for v, t in zip(values(), types):
        assert np.array_equal(v, np.where(t == host.NeumannBoundary, 4.0, 3.0))
    # each physical DoF once: the number of vertex and edge DoFs inside the face z = 1
    g = host.P2Function(st, "g", level, level)
    g.set_boundary_condition(own)
    g.interpolate(1.0, level, host.All)
    keys = set()
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        P = np.concatenate([hu.cell_points(co, level), po.edge_midpoints(co, level)])
        keys |= {bu.point_key(q) for q in P[types[i] == host.NeumannBoundary]}
    assert f.dot(g, level, host.DirichletBoundary) == 4.0 * len(keys) and len(keys) > 0
    # a uid of another condition is refused, not read as a number
    other = host.BoundaryCondition()
    other.create_neumann("elsewhere", 7)
    with pytest.raises(host.HytegHostError, match="belongs to the condition that created it"):
        f.interpolate(5.0, level, boundary_uid=other.boundary_uid(7))
    for o in (f, g, st):
        o.close()


def test_stokes_functions_with_velocity_conditions(env):
    """P1StokesFunction with a condition on w alone, TaylorHoodFunction with one on the whole velocity: the composite's own
    assign / interpolate under DirichletBoundary write, component by component, what that component's condition calls Dirichlet;
    the pressure is all-inner and never written under a boundary flag"""
    torch, host, po, hu, bu, cu = env
    level = 2
    st = bu.outflow_cube()
    own, lid = _lid_condition(host)
    u, five = host.P1StokesFunction(st, "u", level, level), host.P1StokesFunction(st, "five", level, level)
    u.set_velocity_boundary_condition(own, component=2)
    assert u.w.boundary_condition == own and u.u.boundary_condition == host.BoundaryCondition.create_0123()
    assert u.p.boundary_condition == host.BoundaryCondition.create_all_inner()
    for comp in five.components:
        comp.interpolate(5.0, level, host.All)
    u.assign([1.0], [five], level, host.DirichletBoundary)
    for i in range(st.n_local_cells):
        t = bu.point_types(hu.cell_points(st.local_cell(i)[1], level))
        for comp in (u.u, u.v):
            assert np.array_equal(comp.download_cell(i, level), np.where(t == host.DirichletBoundary, 5.0, 0.0))
        assert np.array_equal(u.w.download_cell(i, level), np.where(t == host.NeumannBoundary, 5.0, 0.0))
        assert np.all(u.p.download_cell(i, level) == 0.0)
    u.assign([1.0], [five], level, host.Inner)
    for i in range(st.n_local_cells):
        t = bu.point_types(hu.cell_points(st.local_cell(i)[1], level))
        assert np.array_equal(u.u.download_cell(i, level), np.where(t != host.NeumannBoundary, 5.0, 0.0))
        assert np.array_equal(u.w.download_cell(i, level), np.where(t != host.DirichletBoundary, 5.0, 0.0))
        assert np.all(u.p.download_cell(i, level) == 5.0)
    th = host.TaylorHoodFunction(st, "th", level, level)
    th.set_velocity_boundary_condition(own)
    th.interpolate(3.0, level, host.DirichletBoundary)
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        t = np.concatenate([bu.point_types(hu.cell_points(co, level)), bu.point_types(po.edge_midpoints(co, level))])
        for k in range(3):
            assert th.velocity[k].boundary_condition == own
            assert np.array_equal(np.concatenate(th.velocity[k].download(level, cell=i)), np.where(t == host.NeumannBoundary, 3.0, 0.0))
        assert np.all(th.pressure.download_cell(i, level) == 0.0)
    for o in (th, u, five, st):
        o.close()


def test_dense_coarse_grid_solver_follows_the_velocity_condition(env):
    """DenseCoarseGridSolver assembles identity rows where the boundary condition of the function it solves for fixes a DoF.  Under
    a velocity condition that makes the outflow face a wall too (a closed cavity), the rigid rotation u = ( y - 1/2, 1/2 - x, 0 ),
    p = 0 -- a Stokes solution that lies in P1 -- given on the whole surface is reproduced in the interior, and the values on the
    face z = 1 are kept to the bit (under the storage's default condition they would be unknowns)"""
    torch, host, po, hu, bu, cu = env
    level = 2
    st = bu.outflow_cube(mesh=hu.MESHES / "cube_6el.msh")
    walls = host.BoundaryCondition()
    walls.create_dirichlet("walls", [1, 2])
    L = host.P1P1StokesOperator(st, level, level)
    x, f, r = (host.P1StokesFunction(st, n, level, level) for n in ("x", "f", "r"))
    for fn_ in (x, f, r):
        fn_.set_velocity_boundary_condition(walls)
    flow = [lambda X: X[:, 1] - 0.5, lambda X: 0.5 - X[:, 0], lambda X: 0.0 * X[:, 0]]
    exact, surface = [], []
    for i in range(st.n_local_cells):
        P = hu.cell_points(st.local_cell(i)[1], level)
        surface.append(bu.point_types(P) != host.Inner)
        exact.append([fl(P) for fl in flow])
        for k in range(3):
            x.uvw[k].upload_cell(i, level, np.where(surface[-1], exact[-1][k], 0.0))
    smoother = host.StokesSolver.uzawa(st, level, level, 0.3)
    solver = host.StokesSolver.gmg(st, smoother, level, level, coarse="lu")  # one level: the coarse-grid solver alone
    solver.solve(L, x, f, level)
    err = 0.0
    for i in range(st.n_local_cells):
        for k in range(3):
            got = x.uvw[k].download_cell(i, level)
            assert np.array_equal(got[surface[i]], exact[i][k][surface[i]]), "Dirichlet values, the face z = 1 included, are kept"
            err = max(err, float(np.abs(got - exact[i][k]).max()))
        err = max(err, float(np.abs(x.p.download_cell(i, level)).max()))
    print(f"dense coarse solve under a velocity condition of its own: max error {err:.3e}")
    assert err <= 1e-10  # a direct solve of a system of about 500 unknowns with entries of order one
    for o in (solver, smoother, x, f, r, L, st):
        o.close()


# ---- 11. known answers under the natural boundary condition ---------------------------------------------------------
def _p1_problem(host, hu, bu, st, level, fn):
    """x = u on the Dirichlet points and zero elsewhere, b = 0; returns (x, b, exact cell arrays, selections)"""
    x, b = host.P1Function(st, "x", 2, level), host.P1Function(st, "b", 2, level)
    exact, start = [], []
    for i in range(st.n_local_cells):
        P = hu.cell_points(st.local_cell(i)[1], level)
        u = fn(P[:, 0], P[:, 1], P[:, 2])
        exact.append(u)
        start.append(np.where(bu.point_types(P) == host.DirichletBoundary, u, 0.0))
    hu.upload(x, start, level)
    return x, b, exact


@pytest.mark.parametrize("device_scalars", [True, False])
def test_p1_cg_reproduces_a_linear_harmonic_function_through_the_outflow_face(env, device_scalars):
    torch, host, po, hu, bu, cu = env
    level = 3
    fn = lambda x, y, z: 1.0 + 2.0 * x - 3.0 * y  # noqa: E731 -- harmonic, du/dz = 0, in P1
    errs = {}
    for name in ("outflow", "all Dirichlet"):
        st = bu.outflow_cube() if name == "outflow" else host.Storage.from_gmsh(bu.CUBE)
        A = host.P1ConstantOperator(st, 2, level)
        x, b, exact = _p1_problem(host, hu, bu, st, level, fn)
        cg = host.Solver.cg(st, 2, level, max_iter=1000, tol=1e-14)
        cg.set_use_device_scalars(device_scalars, single_launch=device_scalars)
        cg.solve(A, x, b, level)
        got = hu.download(x, level)
        neumann = [bu.point_types(hu.cell_points(st.local_cell(i)[1], level)) == host.NeumannBoundary for i in range(st.n_local_cells)]
        errs[name] = max(np.abs(g - e).max() for g, e in zip(got, exact))
        on_face = np.concatenate([g[s] for g, s in zip(got, neumann)])
        print(f"{name}, device scalars {device_scalars}: max error {errs[name]:.3e}, {cg.iterations} iterations")
        if name == "outflow":
            assert errs[name] <= 1e-9
        else:  # the counter-check: with the face Dirichlet its interior keeps the start value 0
            assert np.all(on_face == 0.0) and errs[name] > 0.1
        for o in (cg, x, b, A, st):
            o.close()


def test_p1_cg_with_three_exchange_classes_taking_part(env):
    """a second free face (z = 0, flag 4, which create0123BC types Inner): the classes 0, 2 and 4 all take part under
    Inner | NeumannBoundary, one more than the one-launch CG kernel takes group lists for, so the solver goes through the
    multi-launch device CG; u = 1 + 2x - 3y has du/dz = 0 on both faces and is still the answer"""
    torch, host, po, hu, bu, cu = env
    level = 3
    fn = lambda x, y, z: 1.0 + 2.0 * x - 3.0 * y  # noqa: E731
    st = host.Storage.from_gmsh(bu.CUBE)
    st.set_mesh_boundary_flags_by_centroid_location(2, bu.on_outflow)
    st.set_mesh_boundary_flags_by_centroid_location(4, lambda x, y, z: bu.on_outflow(x, y, 1.0 - z))
    assert st.boundary_classes == [0, 1, 2, 4]
    A = host.P1ConstantOperator(st, 2, level)
    x, b = host.P1Function(st, "x", 2, level), host.P1Function(st, "b", 2, level)
    exact, free = [], []
    for i in range(st.n_local_cells):
        P = hu.cell_points(st.local_cell(i)[1], level)
        Pm = P.copy()
        Pm[:, 2] = 1.0 - Pm[:, 2]
        fixed = (bu.point_types(P) == host.DirichletBoundary) & (bu.point_types(Pm) == host.DirichletBoundary)
        assert np.array_equal(hu.point_mask(level, st.mask(i, host.DirichletBoundary)), fixed)
        u = fn(P[:, 0], P[:, 1], P[:, 2])
        x.upload_cell(i, level, np.where(fixed, u, 0.0))
        exact.append(u)
        free.append(~fixed & (np.minimum(P[:, 2], 1.0 - P[:, 2]) < 1e-9))
    assert sum(int(f.sum()) for f in free) > 0
    cg = host.Solver.cg(st, 2, level, max_iter=1000, tol=1e-14)
    cg.set_use_device_scalars(True, single_launch=True)
    cg.solve(A, x, b, level)
    err = max(np.abs(g - e).max() for g, e in zip(hu.download(x, level), exact))
    print(f"two free faces: max error {err:.3e}, {cg.iterations} iterations")
    assert err <= 1e-9
    for o in (cg, x, b, A, st):
        o.close()


def test_p1_multigrid_reduces_the_residual_in_every_cycle_with_a_neumann_part(env):
    torch, host, po, hu, bu, cu = env
    level, flag = 3, host.Inner | host.NeumannBoundary
    st = bu.outflow_cube()
    A = host.P1ConstantOperator(st, 2, level)
    x, b, exact = _p1_problem(host, hu, bu, st, level, lambda x, y, z: 1.0 + 2.0 * x - 3.0 * y)
    r = host.P1Function(st, "r", 2, level)
    gmg = host.Solver.gmg(st, 2, level, smoother=host.GAUSS_SEIDEL, pre=2, post=2)

    def residual():
        A.apply(x, r, level, flag)
        return float(np.sqrt(r.dot(r, level, flag)))

    res = [residual()]
    for _ in range(5):
        gmg.solve(A, x, b, level)
        res.append(residual())
    print("residual norms:", " ".join(f"{v:.3e}" for v in res))
    assert all(res[k + 1] < res[k] for k in range(5))
    assert res[5] < 1e-3 * res[0]
    err = max(np.abs(g - e).max() for g, e in zip(hu.download(x, level), exact))
    assert err < 1e-2  # five cycles: on the way to the known answer, Neumann points included
    for o in (gmg, r, x, b, A, st):
        o.close()


def test_p2_cg_reproduces_a_quadratic_harmonic_function_through_the_outflow_face(env):
    torch, host, po, hu, bu, cu = env
    level = 2
    fn = lambda x, y, z: 1.0 + x * x - y * y  # noqa: E731 -- harmonic, du/dz = 0, in P2
    for name in ("outflow", "all Dirichlet"):
        st = bu.outflow_cube() if name == "outflow" else host.Storage.from_gmsh(bu.CUBE)
        A = host.P2ElementwiseLaplaceOperator(st, level, level)
        x, b = host.P2Function(st, "x", level, level), host.P2Function(st, "b", level, level)
        exact, neumann = [], []
        for i in range(st.n_local_cells):
            co = st.local_cell(i)[1]
            pv, pe = hu.cell_points(co, level), po.edge_midpoints(co, level)
            uv, ue = fn(pv[:, 0], pv[:, 1], pv[:, 2]), fn(pe[:, 0], pe[:, 1], pe[:, 2])
            tv, te = bu.point_types(pv), bu.point_types(pe)
            x.upload(level, np.where(tv == host.DirichletBoundary, uv, 0.0), np.where(te == host.DirichletBoundary, ue, 0.0), cell=i)
            exact.append(np.concatenate([uv, ue]))
            neumann.append(np.concatenate([tv, te]) == host.NeumannBoundary)
        its = A.cg_solve(x, b, level, max_iter=2000, tol=1e-14)
        got = [np.concatenate(x.download(level, cell=i)) for i in range(st.n_local_cells)]
        err = max(np.abs(g - e).max() for g, e in zip(got, exact))
        print(f"P2 {name}: max error {err:.3e}, {its} iterations")
        if name == "outflow":
            assert err <= 1e-9
        else:
            assert all(np.all(g[s] == 0.0) for g, s in zip(got, neumann)) and err > 0.1
        for o in (x, b, A, st):
            o.close()


# ---- 13. two ranks on one GPU ---------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(host, hu, storage, level):
    """apply and one Gauss-Seidel sweep under Inner | NeumannBoundary; {global cell id: array} of each"""
    A = host.P1ConstantOperator(storage, level, level)
    u, r, b = (host.P1Function(storage, n, level, level) for n in ("u", "r", "b"))
    for c in range(storage.n_local_cells):
        P = hu.cell_points(storage.local_cell(c)[1], level)
        u.upload_cell(c, level, np.ascontiguousarray(np.sin(5 * P[:, 0] + 2 * P[:, 1]) + P[:, 2] * P[:, 0]))
    u.sync_shared(level, host.All)
    A.apply(u, r, level, IN)
    applied = {storage.local_cell(c)[0]: r.download_cell(c, level) for c in range(storage.n_local_cells)}
    b.interpolate(1.0, level, host.All)
    A.smooth_gs(u, b, level, IN)
    swept = {storage.local_cell(c)[0]: u.download_cell(c, level) for c in range(storage.n_local_cells)}
    return applied, swept


def _worker(rank, world, port, level, q, transport):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    import bcutil as bu
    import hostutil as hu
    from hyteg_amd import host
    from hyteg_amd.distributed import DistributedContext

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = bu.outflow_cube("centroid", rank, world)
        st.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx = DistributedContext(st, [level], torch.device("cuda", 0), transport=transport)
        assert ctx.class_flags == [0, 1, 2]
        if transport == "p2p":
            assert ctx.transport == "p2p" and st.transport == "p2p", ctx.transport_note
        out = _run(host, hu, st, level)
        st.check_transport()
        q.put((rank,) + out)
        dist.barrier()
    except BaseException as e:  # the parent fails at once instead of waiting for the queue
        q.put(("error", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("transport", ["auto", "p2p"])
def test_two_ranks_on_one_gpu_reproduce_the_one_rank_results(env, transport):
    import torch.multiprocessing as mp

    torch, host, po, hu, bu, cu = env
    level, world = 2, 2
    st = bu.outflow_cube()
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    ref_applied, ref_swept = _run(host, hu, st, level)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, level, q, transport), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    for _ in range(world):
        results.append(q.get(timeout=240))
        assert results[-1][0] != "error", results[-1]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cells = 0
    for rank, applied, swept in results:
        for gid, arr in applied.items():
            assert np.array_equal(arr, ref_applied[gid]), f"apply differs on rank {rank}, cell {gid}"
            cells += 1
        for gid, arr in swept.items():
            assert np.array_equal(arr, ref_swept[gid]), f"Gauss-Seidel sweep differs on rank {rank}, cell {gid}"
    assert cells == st.n_cells
    st.close()
