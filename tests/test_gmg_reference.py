"""CPU pins of tests/gmgutil.py, the global-matrix restatement of the multigrid cycle and of MINRES that test_gpu_gmg_cycles.py and
test_gpu_minres_iterates.py compare the host solvers with: the prolongation against its defining properties and against the
single-cell oracle, the cycle against the independently written one-cell cycle of chebyshevutil and against the two-grid formula on
dense matrices, MINRES against the minimisation that defines it, and the measurement of the rounding that bounds the GPU
comparisons (float64 against 80-bit arithmetic, case by case)."""
import numpy as np
import pytest

import chebyshevutil
import gmgutil as gu
from oracle import p1_oracle as po

LINEAR = lambda p: 42.0 * p[:, 0] + p[:, 1] + 1337.0 * p[:, 2]  # noqa: E731


@pytest.mark.parametrize("mesh,lo,hi,outflow", [("tet_1el", 0, 4, False), ("regular_octahedron_8el", 0, 3, False), ("cube_6el", 1, 3, False),
                                                ("cube_24el", 2, 3, True)])
def test_prolongation_reproduces_linears_and_constants(mesh, lo, hi, outflow):
    h = gu.hierarchy(mesh, lo, hi, outflow)
    for l in range(lo, hi):
        P, C, F = h.P[l], h.levels[l], h.levels[l + 1]
        assert P.shape == (F.glob.ndof, C.glob.ndof)
        assert np.array_equal(np.asarray(P.sum(axis=1)).ravel(), np.ones(F.glob.ndof))  # weights 1 or 1/2 + 1/2: exact
        assert np.array_equal(P @ np.full(C.glob.ndof, 7.5), np.full(F.glob.ndof, 7.5))
        err = np.abs(P @ LINEAR(C.coords) - LINEAR(F.coords)).max() / np.abs(LINEAR(F.coords)).max()
        print(f"{mesh} {l} -> {l + 1}: linear reproduced to {err:.2e}")
        assert err <= 1e-13
        assert np.array_equal(h.restrict(np.ones(F.glob.ndof), l + 1), P.T @ np.ones(F.glob.ndof))


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_prolongation_on_one_cell_is_the_oracles(level):
    h = gu.hierarchy("tet_1el", level, level + 1)
    gc, gf = h.levels[level].glob.gidx[0], h.levels[level + 1].glob.gidx[0]
    P = h.P[level].toarray()
    nnc = np.ones(14)
    for j in range(po.cell_size(level)):
        e = np.zeros(po.cell_size(level))
        e[j] = 1.0
        fine = np.zeros(po.cell_size(level + 1))
        po.prolongate_cell(e, fine, level, nnc)
        assert np.array_equal(P[gf, gc[j]], fine), f"column {j}"


@pytest.mark.parametrize("pre,post", [(1, 1), (3, 3)])
def test_cycle_on_one_cell_equals_the_cell_cycle(pre, post):
    """tet_1el, levels 2-4, Jacobi 2/3: gmgutil.cycle (global matrices, P from geometry) against chebyshevutil.CellCycle (the oracle's
    apply_cell / restrict_cell / prolongate_cell), two restatements written independently of each other"""
    lo, hi, relax = 2, 4, 2.0 / 3.0
    h = gu.hierarchy("tet_1el", lo, hi)
    top = h.levels[hi]
    coords = top.glob.vertices[top.glob.mesh_cells[0]].reshape(12)
    w = {l: po.assemble_cell_stencil(coords, l) for l in range(lo, hi + 1)}

    def smooth(x, b, l):
        dst = x.copy()
        po.jacobi_cell(dst, b, x, l, w[l], relax)
        return dst

    cell = chebyshevutil.CellCycle(coords, lo, hi, smooth, pre, post)
    rng = np.random.default_rng(5)
    inner = cell.inner[hi]
    assert np.array_equal(top.free[top.glob.gidx[0]], inner)
    x_c, b_c = np.where(inner, rng.standard_normal(inner.size), 0.0), np.where(inner, rng.standard_normal(inner.size), 0.0)
    xs = {l: rng.standard_normal(h.levels[l].glob.ndof) for l in range(lo, hi)}  # junk below the top
    bs = {l: np.zeros(h.levels[l].glob.ndof) for l in range(lo, hi)}
    xs[hi], bs[hi] = top.to_global([x_c]), top.to_global([b_c])
    smoother = gu.jacobi_smoother(h, relax)
    for k in range(3):
        x_c = cell.cycle(x_c, b_c)
        gu.cycle(h, smoother, xs, bs, hi, pre, post)
        err = gu.rel(top.to_cells(xs[hi])[0], x_c)
        print(f"V({pre},{post}) cycle {k + 1}: relative L2 difference {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("mesh,outflow", [("cube_6el", False), ("cube_24el", True)])
def test_two_grid_cycle_without_smoothing_is_the_coarse_grid_correction(mesh, outflow):
    """levels 2-3, pre = post = 0: x + P A_c^-1 P^T ( b - A x ) on the free points, with dense matrices"""
    h = gu.hierarchy(mesh, 2, 3, outflow)
    F, C = h.levels[3], h.levels[2]
    assert C.free.sum() > 1
    rng = np.random.default_rng(6)
    x, b = np.where(F.free, rng.standard_normal(F.glob.ndof), 0.0), rng.standard_normal(F.glob.ndof)
    A, Ac, P = F.A.toarray(), C.A.toarray(), h.P[2].toarray()
    Pf = P[np.ix_(F.free, C.free)]
    want = x.copy()
    want[F.free] += Pf @ np.linalg.solve(Ac[np.ix_(C.free, C.free)], Pf.T @ (b - A @ x)[F.free])
    xs, bs = {3: x.copy(), 2: rng.standard_normal(C.glob.ndof)}, {3: b, 2: rng.standard_normal(C.glob.ndof)}
    junk_b = bs[2].copy()
    gu.cycle(h, lambda x, b, l: pytest.fail("no smoothing"), xs, bs, 3, 0, 0)
    assert gu.rel(xs[3], want) <= 1e-13
    assert np.array_equal(xs[3][~F.free], x[~F.free])
    assert np.array_equal(bs[2][~C.free], junk_b[~C.free]) and np.all(xs[2][~C.free] == 0.0)


def test_w_cycle_visits_the_coarser_level_twice():
    """a counting smoother: V(1,2) on levels 1-3 calls it 3 times per level, W(1,2) 3 times on level 3 and 6 times on level 2"""
    h = gu.hierarchy("cube_6el", 1, 3)
    for wcycle, want in ((False, {3: 3, 2: 3}), (True, {3: 3, 2: 6})):
        calls = {3: 0, 2: 0}

        def smooth(x, b, l):
            calls[l] += 1
            return x

        xs = {l: np.zeros(h.levels[l].glob.ndof) for l in (1, 2, 3)}
        bs = {l: np.ones(h.levels[l].glob.ndof) for l in (1, 2, 3)}
        gu.cycle(h, smooth, xs, bs, 3, 1, 2, wcycle)
        assert calls == want


@pytest.mark.parametrize("mesh,level", [("tet_1el", 3), ("regular_octahedron_8el", 2)])
def test_minres_iterates_minimise_the_residual_over_the_krylov_space(mesh, level):
    """identity preconditioner: iterate k minimises || b - A x ||_2 over x0 + K_k( A, r0 ), k = 1..6.  The minimiser is computed
    from an orthonormal basis (Arnoldi with re-orthogonalisation) and a dense least-squares solve: 1e-10 leaves three digits above
    cond( A ) * eps for these matrices (cond < 1e2)"""
    L = gu.global_level(mesh, level)
    f = L.free
    A = L.A.toarray()
    Aff = A[np.ix_(f, f)]
    assert np.linalg.cond(Aff) < 1e2 and f.sum() >= 7
    rng = np.random.default_rng(8)
    x0, b = rng.standard_normal(L.glob.ndof), rng.standard_normal(L.glob.ndof)
    r0 = (b - A @ x0)[f]
    Q = [r0 / np.linalg.norm(r0)]
    for k in range(1, 7):
        x, etas = gu.minres(L.apply, gu.identity_preconditioner(f), x0, b, f, k)
        assert len(etas) == k and np.array_equal(x[~f], x0[~f])
        B = np.stack(Q, axis=1)
        y = np.linalg.lstsq(Aff @ B, r0, rcond=None)[0]
        want = x0[f] + B @ y
        err = np.linalg.norm(x[f] - want) / np.linalg.norm(want - x0[f])
        res = np.linalg.norm(r0 - Aff @ (x[f] - x0[f]))
        print(f"{mesh} k = {k}: iterate against the minimiser {err:.2e}, residual {res:.6e}, |eta| {abs(etas[-1]):.6e}")
        assert err <= 1e-10
        assert abs(abs(etas[-1]) - res) <= 1e-10 * np.linalg.norm(r0)  # |eta| is the residual norm MINRES carries along
        q = Aff @ Q[-1]
        for _ in range(2):
            for p in Q:
                q = q - (p @ q) * p
        Q.append(q / np.linalg.norm(q))


def test_jacobi_preconditioner_in_closed_form():
    """x = r, then m = 2 steps x += D^-1 ( r - A x ) is  N^2 r + ( I + N ) D^-1 r  with N = I - D^-1 A, on dense matrices"""
    L = gu.global_level("regular_octahedron_8el", 2)
    f = L.free
    A, D = L.A.toarray()[np.ix_(f, f)], L.D[f]
    r = np.random.default_rng(9).standard_normal(L.glob.ndof)
    N = np.eye(len(D)) - A / D[:, None]
    want = N @ N @ r[f] + (np.eye(len(D)) + N) @ (r[f] / D)
    got = gu.jacobi_preconditioner(L, 2)(np.where(f, r, 0.0))
    assert gu.rel(got[f], want) <= 1e-13 and np.all(got[~f] == 0.0)
    assert np.array_equal(gu.jacobi_preconditioner(L, 0)(np.where(f, r, 0.0)), np.where(f, r, 0.0))


# ---- the tolerance of the GPU comparisons: measured here, on the restatement alone -----------------------------------
@pytest.mark.parametrize("case", gu.GMG_CASES, ids=gu.case_id)
def test_rounding_of_the_restated_cycles(case):
    """float64 against 80-bit: d <= 1e-12, so the GPU bound 1e-12 + 50 d never exceeds 5.1e-11; and the three cycles do something"""
    assert np.finfo(np.longdouble).eps < 2e-19
    r = gu.restated(case)
    x0 = gu.case_inputs(case)[0][case.hi]
    print(f"{gu.case_id(case)}: d_x = {r.d_x:.2e}, d_b = {r.d_b:.2e}; bounds {gu.tolerance(r.d_x):.2e}, {gu.tolerance(r.d_b):.2e}")
    assert r.d_x <= 1e-12 and r.d_b <= 1e-12
    assert gu.rel(r.iterates[0], x0) > 0.1 and all(gu.rel(a, b) > 1e-6 for a, b in zip(r.iterates[1:], r.iterates[:-1]))
    assert all(np.linalg.norm(b) > 0 for b in r.b_lower.values())


@pytest.mark.parametrize("case", gu.MINRES_CASES, ids=gu.minres_id)
def test_rounding_of_the_restated_minres(case):
    r = gu.minres_restated(case)
    print(f"{gu.minres_id(case)}: d_x = {r.d_x:.2e}; bound {gu.tolerance(r.d_x):.2e}; |eta| {[f'{abs(e):.3e}' for e in r.etas]}")
    assert r.d_x <= 1e-12 and len(r.etas) == case.k
    assert all(abs(b) < abs(a) for a, b in zip(r.etas[:-1], r.etas[1:]))  # the carried residual norm falls
