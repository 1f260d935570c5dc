"""Pins the CPU restatement of -div( k grad u ) (tests/divkgradutil.py) that the GPU tests of P1ElementwiseDivKGrad compare with:
to the reference's Laplace element matrices, to the constant-stencil apply for k = 1, and to the reference's known answer
(tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp).  CPU only."""
import numpy as np
import pytest

import divkgradutil as dk
import ref_golden
from conftest import OCT_TET, REF_TET, SKEW_TET
from oracle import p1_oracle as po


@pytest.mark.parametrize("tet", [REF_TET, OCT_TET, SKEW_TET])
def test_element_matrix_is_the_references_laplace_matrix(tet):
    ref = ref_golden.ref_fenics()
    c = np.asarray(tet, dtype=np.float64).reshape(12)
    A = np.empty(16)
    ref.ref_p1_tet_diffusion(po._p(A), po._p(c))
    K = dk.laplace_element_matrix(tet)
    assert np.abs(K - A.reshape(4, 4)).max() <= 2e-14 * np.abs(A).max()  # the bound of the existing Laplace pins
    assert np.abs(K.sum(axis=1)).max() <= 1e-15 * np.abs(K).max() * 4


def test_indexing_and_classes_match_the_oracle():
    for level in (0, 1, 2, 3):
        assert dk.cell_size(level) == po.cell_size(level)
        assert np.array_equal(dk.cell_coords(level), po.cell_coords(level))
        assert np.array_equal(dk.point_slots(level), po.slot_of_points(level))
        c = dk.cell_coords(level)
        assert np.array_equal(dk.cell_index(level, c[:, 0], c[:, 1], c[:, 2]), np.arange(len(c)))
    # 6 types tile the macro-cell: 8^level micro-cells
    assert sum(len(dk.micro_cells(3, t)) for t in range(6)) == 8 ** 3


@pytest.mark.parametrize("tet", [SKEW_TET, OCT_TET])
@pytest.mark.parametrize("level", [2, 3])
def test_unit_coefficient_equals_the_stencil_apply(tet, level):
    """k = 1: the elementwise sum equals the constant-stencil apply at the inner points and at every shell class, to the reference's
    own elementwise-versus-stencil criterion (1e-13, P1JacobiConvergenceTest.cpp:117)"""
    rng = np.random.default_rng(level)
    n = dk.cell_size(level)
    src = rng.uniform(-1.0, 1.0, n)
    mine = dk.apply_cell(src, np.ones(n), tet, level)
    ref = np.zeros(n)
    po.apply_cell(ref, src, level, po.assemble_cell_stencil(tet, level))
    po.apply_cell_boundary(ref, src, level, po.assemble_cell_slot_stencils(tet, level), po.MASK_SHELL)
    slots = dk.point_slots(level)
    for cls in range(15):
        sel = slots == cls
        assert sel.any()
        assert np.abs(mine[sel] - ref[sel]).max() <= 1e-13 * np.abs(ref).max(), cls
    # the class mask restricts, the diagonal is the stencil's centre weight
    only = dk.apply_cell(src, np.ones(n), tet, level, mask=1 << 7)
    assert np.array_equal(only[slots == 7], mine[slots == 7]) and not only[slots != 7].any()
    w = np.asarray(po.assemble_cell_stencil(tet, level))
    d = dk.diagonal_cell(np.ones(n), tet, level)
    assert np.abs(d[slots == 14] - w[7]).max() <= 1e-13 * abs(w[7])


def test_dense_assembly_is_the_element_loop():
    level, tet = 2, SKEW_TET
    rng = np.random.default_rng(5)
    n = dk.cell_size(level)
    src, k = rng.uniform(-1, 1, n), rng.uniform(0.5, 2.0, n)
    A = dk.dense_cell(k, tet, level)
    assert np.abs(A @ src - dk.apply_cell(src, k, tet, level)).max() <= 1e-14 * np.abs(A).max() * 15
    assert np.abs(A - A.T).max() == 0.0
    assert np.abs(np.diag(A) - dk.diagonal_cell(k, tet, level)).max() <= 1e-15 * np.abs(A).max() * 24


@pytest.mark.parametrize("level", [3, 4])
def test_known_answer_of_the_reference_by_a_dense_solve(level):
    """tet_1el, k = tanh( 2 ( x - 0.5 ) ) + 2, u = sin( 2 pi x ) sinh( pi y ), right-hand side M * ( the reference's rhs ), Dirichlet
    values on the whole boundary; error normalised by the P2 DoF count as the reference does (dk.known_error)"""
    p = dk.cell_points(REF_TET, level)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    k = dk.known_k(x, y, z)
    A = dk.dense_cell(k, REF_TET, level)
    f = dk.dense_cell(None, REF_TET, level, mass=True) @ dk.known_rhs(x, y, z)
    inner = dk.point_slots(level) == 14
    u = dk.known_u(x, y, z)
    u[inner] = 0.0
    u[inner] = np.linalg.solve(A[np.ix_(inner, inner)], f[inner] - A[np.ix_(inner, ~inner)] @ u[~inner])
    err = dk.known_error(u, REF_TET, level)
    print(f"level {level}: discrete L2 error {err:.3e} (bound {dk.KNOWN_BOUNDS[level]:.1e})")
    assert err < dk.KNOWN_BOUNDS[level]
    # the bound discriminates: the plain Laplacian with the same right-hand side misses it by an order of magnitude
    L = dk.dense_cell(np.ones_like(k), REF_TET, level)
    v = dk.known_u(x, y, z)
    v[inner] = np.linalg.solve(L[np.ix_(inner, inner)], f[inner] - L[np.ix_(inner, ~inner)] @ v[~inner])
    assert dk.known_error(v, REF_TET, level) > 4 * dk.KNOWN_BOUNDS[level]
