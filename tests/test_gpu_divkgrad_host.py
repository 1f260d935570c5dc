"""GPU tests of the host-layer class P1ElementwiseDivKGrad and its solvers (hyteg_amd/host/p1divkgrad.hpp, host.DivKGradSolver)
against the numpy element loop of tests/divkgradutil.py per macro-cell plus hostutil.MultiCellOracle.sum_shared for the shared
points, and against the reference's known answer (tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp)."""
from pathlib import Path

import numpy as np
import pytest

import divkgradutil as dk
from conftest import REF_TET

pytestmark = pytest.mark.gpu
MESHES = Path(__file__).resolve().parent.parent / "hyteg_amd" / "data" / "meshes"


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


def storage(env, mesh):
    torch, host, hu = env
    st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    return st


def field(seed):
    """a smooth function with seeded coefficients: evaluated per cell it has the same value on every copy of a shared point"""
    a = np.random.default_rng(seed).uniform(1.0, 4.0, 6)
    return lambda x, y, z: np.sin(a[0] * x + a[1] * y) * np.cos(a[2] * z + a[3]) + 0.3 * np.cos(a[4] * y - a[5] * x)


def coefficient(seed):
    f = field(seed)
    return lambda x, y, z: 1.25 + 0.6 * f(x, y, z)  # within [0.47, 2.03]


def function(env, st, name, lo, hi, arrays_by_level):
    torch, host, hu = env
    f = host.P1Function(st, name, lo, hi)
    for level, arrays in arrays_by_level.items():
        hu.upload(f, arrays, level)
    return f


def rel(a, b):
    a, b = np.concatenate(a), np.concatenate(b)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def restated_apply(orc, st, u, k, prior, level, flag):
    """per cell: the element loop on the classes the flag selects; then the shares of shared points are summed"""
    out = [p.copy() for p in prior]
    sels = []
    for i, (gid, co, nnc) in enumerate(orc.cells):
        sel = dk.point_mask(level, st.mask(i, flag))
        out[i][sel] = dk.apply_cell(u[i], k[i], co, level)[sel]
        sels.append(sel)
    orc.sum_shared(out, level, flag)
    return out, sels


@pytest.mark.parametrize("level", [2, 3])
@pytest.mark.parametrize("mesh", ["cube_6el", "regular_octahedron_8el"])
def test_apply_on_several_cells(env, mesh, level):
    torch, host, hu = env
    st = storage(env, mesh)
    orc = hu.MultiCellOracle(st)
    u_h, k_h = orc.interpolate(field(1), level), orc.interpolate(coefficient(2), level)
    prior = orc.interpolate(field(3), level)
    u, k = function(env, st, "u", level, level, {level: u_h}), function(env, st, "k", level, level, {level: k_h})
    A = host.P1ElementwiseDivKGrad(st, level, level, k)
    for flag in (host.All, host.Inner):
        dst = function(env, st, "dst", level, level, {level: prior})
        A.apply(u, dst, level, flag)
        want, sels = restated_apply(orc, st, u_h, k_h, prior, level, flag)
        got = hu.download(dst, level)
        err = rel([g[s] for g, s in zip(got, sels)], [w[s] for w, s in zip(want, sels)])
        print(f"{mesh} level {level} flag {flag}: relative L2 error {err:.3e}")
        assert err <= 1e-12
        for g, p, s in zip(got, prior, sels):
            assert np.array_equal(g[~s], p[~s]), "points the flag does not select keep their contents"
        # Add: on several cells the shares go through the scratch function
        A.apply(u, dst, level, flag, host.Add)
        got2 = hu.download(dst, level)
        twice = [np.where(s, 2.0 * w, w) for w, s in zip(want, sels)]
        assert rel([g[s] for g, s in zip(got2, sels)], [w[s] for w, s in zip(twice, sels)]) <= 1e-12
        dst.close()
    for o in (A, u, k, st):
        o.close()


def test_operator_is_symmetric(env):
    """< A u, v > = < u, A v > on cube_6el, level 3"""
    torch, host, hu = env
    level = 3
    st = storage(env, "cube_6el")
    orc = hu.MultiCellOracle(st)
    fs = {n: function(env, st, n, level, level, {level: orc.interpolate(f, level)})
          for n, f in (("u", field(11)), ("v", field(12)), ("k", coefficient(13)))}
    au, av = host.P1Function(st, "au", level, level), host.P1Function(st, "av", level, level)
    A = host.P1ElementwiseDivKGrad(st, level, level, fs["k"])
    A.apply(fs["u"], au, level, host.All)
    A.apply(fs["v"], av, level, host.All)
    lhs, rhs = au.dot(fs["v"], level, host.All), fs["u"].dot(av, level, host.All)
    print(f"< A u, v > = {lhs:.15e}, < u, A v > = {rhs:.15e}")
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * abs(lhs)
    for o in (A, au, av, *fs.values(), st):
        o.close()


@pytest.mark.parametrize("mesh,level", [("cube_6el", 3), ("tet_1el", 4)])
def test_constant_coefficient_is_a_multiple_of_the_diffusion_operator(env, mesh, level):
    """k = 3 equals 3 * P1ElementwiseDiffusion.apply, to 1e-13"""
    torch, host, hu = env
    st = storage(env, mesh)
    orc = hu.MultiCellOracle(st)
    u = function(env, st, "u", level, level, {level: orc.interpolate(field(21), level)})
    k, a, b = (host.P1Function(st, n, level, level) for n in ("k", "a", "b"))
    k.interpolate(3.0, level, host.All)
    A, L = host.P1ElementwiseDivKGrad(st, level, level, k), host.P1ElementwiseDiffusion(st, level, level)
    A.apply(u, a, level, host.All)
    L.apply(u, b, level, host.All)
    got, lap = hu.download(a, level), [3.0 * x for x in hu.download(b, level)]
    assert rel(got, lap) <= 1e-13
    assert max(np.abs(g - w).max() for g, w in zip(got, lap)) <= 1e-13 * max(np.abs(w).max() for w in lap)
    for o in (A, L, u, k, a, b, st):
        o.close()


def test_boundary_condition_of_the_destination_is_honoured(env):
    """one macro-face carries mesh flag 2: a destination whose own condition makes flag 2 a Neumann boundary gets the face written
    under Inner | NeumannBoundary, one whose condition makes it a Dirichlet boundary does not"""
    torch, host, hu = env
    level = 3
    st = host.Storage.single_tet(REF_TET)
    face = [i for i in range(st.n_faces) if st.primitive(2, i).vertex_ids == (0, 1, 2)]
    st.set_mesh_boundary_flag(2, face[0], 2)
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    orc = hu.MultiCellOracle(st)
    u_h, k_h, prior = (orc.interpolate(f, level) for f in (field(31), coefficient(32), field(33)))
    u, k = function(env, st, "u", level, level, {level: u_h}), function(env, st, "k", level, level, {level: k_h})
    A = host.P1ElementwiseDivKGrad(st, level, level, k)
    flag = host.Inner | host.NeumannBoundary
    ref = dk.apply_cell(u_h[0], k_h[0], REF_TET, level)
    on_face = dk.point_mask(level, 1 << 6)
    for neumann in (True, False):
        bc = host.BoundaryCondition()
        if neumann:
            bc.create_dirichlet("walls", 1)
            bc.create_neumann("open", [2])
        else:
            bc.create_dirichlet("walls", [1, 2])
        dst = function(env, st, "dst", level, level, {level: prior})
        dst.set_boundary_condition(bc)
        mask = st.mask(0, flag, bc=bc)
        assert mask == (dk.MASK_INNER | (1 << 6) if neumann else dk.MASK_INNER)
        A.apply(u, dst, level, flag)
        got, sel = dst.download_cell(0, level), dk.point_mask(level, mask)
        assert np.abs(got[sel] - ref[sel]).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(got[~sel], prior[0][~sel])
        assert np.array_equal(got[on_face], prior[0][on_face]) != neumann  # the flagged face was written / was left alone
        dst.close()
    for o in (A, u, k, st):
        o.close()


def test_inverse_diagonal_is_the_diagonal_of_the_global_matrix(env):
    torch, host, hu = env
    level = 2
    st = storage(env, "cube_6el")
    orc = hu.MultiCellOracle(st)
    vertices, cells = hu.read_msh(MESHES / "cube_6el.msh")
    assert [c[0] for c in orc.cells] == list(range(len(cells)))
    k_h = orc.interpolate(coefficient(41), level)
    k = function(env, st, "k", level, level, {level: k_h})
    A = host.P1ElementwiseDivKGrad(st, level, level, k)
    with pytest.raises(host.HytegHostError, match="Inverse diagonal values have not been assembled"):
        A.inverse_diagonal()
    A.compute_inverse_diagonal_operator_values()
    G, gidx = dk.dense_global(vertices, cells, k_h, level)
    assert np.abs(G - G.T).max() <= 1e-15 * np.abs(G).max()
    got = hu.download(A.inverse_diagonal(), level)
    for c in range(len(cells)):
        want = 1.0 / np.diag(G)[gidx[c]]
        assert np.abs(got[c] - want).max() <= 1e-12 * np.abs(want).max()
    for o in (A, k, st):
        o.close()


@pytest.mark.parametrize("mesh,level", [("cube_6el", 3), ("tet_1el", 4)])
def test_smooth_jac_fused_and_composed(env, mesh, level):
    """the fused step agrees with the composed four passes to 1e-13, the composed form with their numpy statement"""
    torch, host, hu = env
    st = storage(env, mesh)
    orc = hu.MultiCellOracle(st)
    src_h, rhs_h, k_h, prior = (orc.interpolate(f, level) for f in (field(51), field(52), coefficient(53), field(54)))
    src, rhs, k = (function(env, st, n, level, level, {level: a}) for n, a in (("src", src_h), ("rhs", rhs_h), ("k", k_h)))
    A = host.P1ElementwiseDivKGrad(st, level, level, k)
    A.compute_inverse_diagonal_operator_values()
    inv = hu.download(A.inverse_diagonal(), level)
    omega = 0.6
    for flag in (host.Inner, host.All):
        out = {}
        for fused in (True, False):
            A.set_fused(fused)
            dst = function(env, st, "dst", level, level, {level: prior})
            A.smooth_jac(dst, rhs, src, omega, level, flag)
            out[fused] = hu.download(dst, level)
            dst.close()
        A.set_fused(True)
        asrc, sels = restated_apply(orc, st, src_h, k_h, prior, level, flag)
        want = [np.where(s, u + omega * (d * (r - a)), p) for s, u, d, r, a, p in zip(sels, src_h, inv, rhs_h, asrc, prior)]
        assert rel(out[False], want) <= 1e-12
        assert rel(out[True], out[False]) <= 1e-13
        for g, p, s in zip(out[True], prior, sels):
            assert np.array_equal(g[~s], p[~s])
    for o in (A, src, rhs, k, st):
        o.close()


def known_answer_setup(env, st, lo, hi):
    """k on every level, f = M * rhs and the Dirichlet values of the exact solution on the top level"""
    torch, host, hu = env
    orc = hu.MultiCellOracle(st)
    k = function(env, st, "k", lo, hi, {l: orc.interpolate(dk.known_k, l) for l in range(lo, hi + 1)})
    r = function(env, st, "r", hi, hi, {hi: orc.interpolate(dk.known_rhs, hi)})
    f = host.P1Function(st, "f", lo, hi)
    M = host.P1ConstantOperator(st, hi, hi, form=1)
    M.apply(r, f, hi, host.All)
    exact = orc.interpolate(dk.known_u, hi)
    start = []
    for i, e in enumerate(exact):
        inner = dk.point_mask(hi, st.mask(i, host.Inner))
        start.append(np.where(inner, 0.0, e))
    for o in (M, r):
        o.close()
    return orc, k, f, exact, start


@pytest.mark.parametrize("level", [3, 4, 5])
def test_known_answer_of_the_reference_by_cg(env, level):
    """tet_1el, levels 3, 4, 5, CGSolver( 1000, 1e-12 ): the reference's functions, normalisation (dk.known_error: the P2 DoF
    count) and bounds 2.5e-3, 7.2e-4, 2.0e-4"""
    torch, host, hu = env
    max_iter = 1000
    st = storage(env, "tet_1el")
    orc, k, f, exact, start = known_answer_setup(env, st, level, level)
    tet = orc.cells[0][1]  # the mesh file's node order, not REF_TET's
    u = function(env, st, "u", level, level, {level: start})
    A = host.P1ElementwiseDivKGrad(st, level, level, k)
    cg = host.DivKGradSolver.cg(st, level, level, max_iter=max_iter, tol=1e-12)
    cg.solve(A, u, f, level)
    err = dk.known_error(u.download_cell(0, level), tet, level)
    print(f"level {level}: discrete L2 error {err:.3e} (bound {dk.KNOWN_BOUNDS[level]:.1e}), {cg.iterations} CG iterations")
    assert 0 < cg.iterations < max_iter
    assert err < dk.KNOWN_BOUNDS[level]
    for o in (cg, A, u, k, f, st):
        o.close()


def residual(env, st, orc, A, x, b_h, level):
    """|| b - A x || / || b || over the inner points, with the library's apply and numpy's norms"""
    torch, host, hu = env
    t = host.P1Function(st, "t", level, level)
    A.apply(x, t, level, host.Inner)
    ax = hu.download(t, level)
    t.close()
    sels = [dk.point_mask(level, st.mask(i, host.Inner)) for i in range(len(b_h))]
    r = [np.where(s, b - a, 0.0) for s, b, a in zip(sels, b_h, ax)]
    bb = [np.where(s, b, 0.0) for s, b in zip(sels, b_h)]
    return float(np.sqrt(orc.dot(r, r, level, host.Inner) / orc.dot(bb, bb, level, host.Inner)))


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_multigrid_preconditioned_cg(env, smoother):
    """cube_6el, levels 2-4, k of the known answer on every level: CG preconditioned by one V(2,2) cycle reaches a relative residual
    of 1e-10, agrees with unpreconditioned CG at the same tolerance to 1e-8 and takes fewer iterations (no count is fixed in advance;
    recorded on the MI355X: see DESIGN.md)"""
    torch, host, hu = env
    lo, hi, tol = 2, 4, 1e-10
    st = storage(env, "cube_6el")
    orc, k, f, exact, start = known_answer_setup(env, st, lo, hi)
    b_h = hu.download(f, hi)
    A = host.P1ElementwiseDivKGrad(st, lo, hi, k)
    A.compute_inverse_diagonal_operator_values()
    if smoother == "jacobi":
        gmg = host.DivKGradSolver.gmg(st, lo, hi, smoother=host.JACOBI, relax=2.0 / 3.0, pre=2, post=2)
    else:
        radii = []
        for l in range(lo, hi + 1):
            v = function(env, st, "v", l, l, {l: orc.interpolate(lambda x, y, z: 1.0 + np.sin(5 * x + y) * np.cos(3 * z), l)})
            t = host.P1Function(st, "t", l, l)
            radii.append(host.estimate_radius(A, l, 30, v, t))
            v.close()
            t.close()
        print("spectral radii of D^-1 A:", radii)
        assert all(0.0 < r <= 4.0 for r in radii)  # D^-1 A of four-node elements: eigenvalues in ( 0, 4 ]
        gmg = host.DivKGradSolver.gmg_chebyshev(st, lo, hi, 2, radii, pre=2, post=2)
    zero = [np.zeros_like(s) for s in start]  # homogeneous Dirichlet values: the right-hand side alone drives the solve
    x_pcg, x_cg = function(env, st, "xp", lo, hi, {hi: zero}), function(env, st, "xc", lo, hi, {hi: zero})
    pcg = host.DivKGradSolver.cg(st, lo, hi, max_iter=200, tol=tol, preconditioner=gmg)
    cg = host.DivKGradSolver.cg(st, hi, hi, max_iter=2000, tol=tol)
    pcg.solve(A, x_pcg, f, hi)
    cg.solve(A, x_cg, f, hi)
    res_pcg, res_cg = residual(env, st, orc, A, x_pcg, b_h, hi), residual(env, st, orc, A, x_cg, b_h, hi)
    print(f"{smoother}: preconditioned CG {pcg.iterations} iterations (residual {res_pcg:.2e}), plain CG {cg.iterations} ({res_cg:.2e})")
    assert res_pcg <= tol
    if smoother == "jacobi":
        assert rel(hu.download(x_pcg, hi), hu.download(x_cg, hi)) <= 1e-8
        assert 0 < pcg.iterations < cg.iterations < 2000
    for o in (pcg, cg, gmg, A, x_pcg, x_cg, k, f, st):
        o.close()
