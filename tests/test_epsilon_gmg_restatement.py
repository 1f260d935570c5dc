"""CPU-only: the restatement the GPU tests of the epsilon-operator multigrid cycle and of the block-preconditioned MINRES compare
with (tests/epsilongmgutil.py: gmgutil's Hierarchy, cycle, smoothers and MINRES loop on the dense matrices of tests/epsilonutil.py,
prolongation I_3 (x) P on component-major vectors) is pinned before anything is compared with it, and its own rounding is measured
case by case: every case runs in float64 and in numpy.longdouble, d is the largest relative L2 difference, asserted <= 1e-12 (as
tests/test_gmg_reference.py does) and printed.  The GPU comparisons are bounded by gmgutil.tolerance( d ) = 1e-12 + 50 d."""
import numpy as np
import pytest

import epsilongmgutil as egu
import epsilonutil as eu
import gmgutil as gm


def test_vector_prolongation_reproduces_a_linear_vector_field():
    h = egu.epsilon_hierarchy("cube_6el", 1, 3)
    M, t = np.array([[0.3, -1.1, 0.7], [0.9, 0.4, -0.6], [-0.2, 0.8, 1.3]]), np.array([0.5, -0.25, 2.0])
    field = {l: (h.levels[l].base.coords @ M.T + t).T.reshape(-1) for l in (1, 2, 3)}  # component-major
    for l in (1, 2):
        got = h.prolongate(field[l], l)
        assert np.abs(got - field[l + 1]).max() <= 1e-14 * np.abs(field[l + 1]).max()


def test_restriction_is_the_transpose_of_the_prolongation():
    h = egu.epsilon_hierarchy("tet_1el", 2, 4)
    rng = np.random.default_rng(0)
    for l in (2, 3):
        u, r = rng.standard_normal(3 * h.levels[l].n), rng.standard_normal(3 * h.levels[l + 1].n)
        assert abs(h.prolongate(u, l) @ r - u @ h.restrict(r, l + 1)) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(r)
        assert np.array_equal(h.restrict(r, l + 1), h.P[l].T @ r)
        n_c, n_f = h.levels[l].n, h.levels[l + 1].n
        for k in range(3):  # component k of the coarse vector reaches component k of the fine one only
            e = np.zeros(3 * n_c)
            e[k * n_c:(k + 1) * n_c] = rng.standard_normal(n_c)
            fine = h.prolongate(e, l).reshape(3, n_f)
            assert np.any(fine[k]) and not np.any(np.delete(fine, k, axis=0))


def test_galerkin_product_equals_the_coarse_matrix_for_unit_viscosity():
    """P^T A_fine P = A_coarse with mu = 1: the P1 spaces are nested and the element matrices exact"""
    for mesh, lo, hi in (("cube_6el", 1, 3), ("tet_1el", 2, 3)):
        h = egu.epsilon_hierarchy(mesh, lo, hi, "one")
        for l in range(lo, hi):
            G = (h.P[l].T @ h.levels[l + 1].A @ h.P[l]).toarray()
            A = h.levels[l].A.toarray()
            err = np.abs(G - A).max() / np.abs(A).max()
            print(f"{mesh} {l + 1} -> {l}: max entry difference / max |A| {err:.3e}")
            assert err <= 1e-12


@pytest.mark.parametrize("smoother,param,pre", [("chebyshev", 2, 1), ("jacobi", 2.0 / 3.0, 2)])
def test_restated_cycle_is_a_symmetric_positive_definite_map(smoother, param, pre):
    """the cycle from zero applied to the unit vectors of the free points on cube_6el 1-2, contrast-40 viscosity: what MINRES needs
    of the velocity action"""
    h = egu.epsilon_hierarchy("cube_6el", 1, 2)
    action = egu.cycle_action(h, egu.smoother(h, smoother, param, egu.case_radii("cube_6el", 1, 2)), pre, pre)
    free = np.flatnonzero(h.levels[2].free)
    assert len(free) == 81
    B = np.zeros((len(free), len(free)))
    for j, g in enumerate(free):
        e = np.zeros(3 * h.levels[2].n)
        e[g] = 1.0
        z = action(e)
        assert not np.any(z[~h.levels[2].free])
        B[:, j] = z[free]
    asym = np.abs(B - B.T).max() / np.abs(B).max()
    low = np.linalg.eigvalsh(0.5 * (B + B.T)).min()
    print(f"{smoother}: asymmetry {asym:.3e}, smallest eigenvalue {low:.3e}")
    assert asym <= 1e-13
    assert low > 0.0


@pytest.mark.parametrize("c", egu.CYCLE_CASES, ids=egu.cycle_id)
def test_cycle_cases_in_two_precisions(c):
    r = egu.restated_cycles(c)
    print(f"{egu.cycle_id(c)}: d {r.d:.3e}, residual reductions {[f'{x:.4f}' for x in r.rates]} (d of the reductions {r.d_rate:.3e})")
    assert r.d <= 1e-12 and r.d_rate <= 1e-12
    assert all(0.0 < x < 1.0 for x in r.rates)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mesh,lo,hi", [("cube_6el", 1, 3), ("tet_1el", 2, 4)])
def test_smoother_call_in_two_precisions(mesh, lo, hi, order):
    a, w = egu.smoother_call(mesh, lo, hi, order), egu.smoother_call(mesh, lo, hi, order, gm.LD)
    d = max(gm.rel(a[2], w[2]), gm.rel(a[3], w[3]))
    print(f"{mesh} Chebyshev({order}): d {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("k", egu.MINRES_KS)
@pytest.mark.parametrize("kind", ["block", "block_viscosity"])
def test_block_minres_cases_in_two_precisions(kind, k):
    x, d = egu.restated_minres(kind, k)
    S, free, exact, b, start, lumped, n = egu.minres_problem()
    print(f"{kind} k={k}: d {d:.3e}; moved x by {gm.rel(x[free], start[free]):.2e}")
    assert d <= 1e-12
    assert np.array_equal(x[~free], start[~free])


def test_block_preconditioner_beats_the_pressure_preconditioner_in_the_restated_loop():
    """iterations to 1e-8 of the restated loop: the count the GPU test compares with"""
    S, free, exact, b, start, lumped, n = egu.minres_problem()
    _, etas = egu.run_minres("block", 2000, rel_tol=1e-8)
    scale = np.ones(4 * n)
    scale[3 * n:] = 1.0 / lumped
    _, etas_p = gm.minres(lambda u: S @ u, lambda r: np.where(free, scale * r, 0), start, b, free, 2000, 1e-8)
    print(f"restated MINRES to 1e-8: block {len(etas) - 1}, pressure {len(etas_p) - 1} iterations")
    assert 0 < len(etas) - 1 < len(etas_p) - 1


def test_dense_stokes_matrix_carries_the_epsilon_block():
    S, free, exact, b, start, lumped, n = egu.minres_problem()
    h = egu.epsilon_hierarchy(egu.MINRES_MESH, egu.MINRES_LO, egu.MINRES_LEVEL)
    assert np.array_equal(S[:3 * n, :3 * n], h.levels[egu.MINRES_LEVEL].A.toarray())
    assert eu.cell_size(egu.MINRES_LEVEL) == 35
