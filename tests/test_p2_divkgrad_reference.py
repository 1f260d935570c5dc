"""CPU-only: the numpy restatement of the P2 operator -div( k grad u ) with a P2 coefficient (tests/p2divkgradutil.py) is pinned
against the recorded FEniCS element matrices, against analytic integrals worked out in Cartesian monomials, and against the known
answer of the reference's test (ElementwiseDivKGradCGConvergenceTest.cpp, runAllTestsP2) through a direct solve."""
import itertools
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import gmgutil
import p2divkgradutil as pu

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_fenics_forms.npz"
# a tetrahedron with three different axis lengths: int_T x^a y^b z^c = 2^(a+1) 3^(b+1) a! b! c! / ( a + b + c + 3 )!
BOX_TET = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 1.0]])


def test_constant_coefficient_reproduces_the_recorded_fenics_matrices():
    g = np.load(GOLDEN)
    coords, out = g["ref_p2_tet_diffusion__coords"], g["ref_p2_tet_diffusion__out"]
    assert len(coords) >= 1
    for c, ref in zip(coords, out):
        A = pu.element_matrix(c.reshape(4, 3), np.ones(10))
        assert np.abs(A - ref.reshape(10, 10)).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("seed", range(3))
def test_symmetry_and_zero_row_sums_for_random_positive_coefficients(seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (4, 3))
    A = pu.element_matrix(c, rng.uniform(0.5, 2.0, 10))
    scale = np.abs(A).max()
    assert np.abs(A - A.T).max() <= 1e-14 * scale
    assert np.abs(A.sum(axis=1)).max() <= 1e-13 * scale


# ---- polynomials in x, y, z: { (a, b, c): Fraction } ----
def _pmul(p, q):
    out = {}
    for (ea, ca), (eb, cb) in itertools.product(p.items(), q.items()):
        e = tuple(x + y for x, y in zip(ea, eb))
        out[e] = out.get(e, 0) + ca * cb
    return out


def _pdiff(p, r):
    out = {}
    for e, c in p.items():
        if e[r]:
            d = list(e)
            d[r] -= 1
            out[tuple(d)] = out.get(tuple(d), 0) + c * e[r]
    return out


def _integral_box_tet(p):
    f = math.factorial
    return sum(c * Fraction(2 ** (e[0] + 1) * 3 ** (e[1] + 1) * f(e[0]) * f(e[1]) * f(e[2]), f(sum(e) + 3)) for e, c in p.items())


def _value(p, x):
    return float(sum(c * x[0] ** e[0] * x[1] ** e[1] * x[2] ** e[2] for e, c in p.items()))


def _nodal(p, tet):
    pts = [tet[a] for a in range(4)] + [(tet[a] + tet[b]) / 2.0 for a, b in pu.EDGE_PAIRS]
    return np.array([_value(p, x) for x in pts])


F = Fraction
U = {(2, 0, 0): F(1), (0, 1, 1): F(1), (1, 0, 0): F(-1, 2)}            # x^2 + y z - x / 2
V = {(1, 1, 0): F(1), (0, 0, 2): F(2), (0, 0, 0): F(3)}                # x y + 2 z^2 + 3
K = {(0, 0, 0): F(1), (1, 0, 0): F(1, 2), (0, 2, 0): F(1, 3), (1, 0, 1): F(1)}  # 1 + x / 2 + y^2 / 3 + x z


def test_bilinear_form_equals_the_analytic_integral_for_quadratics():
    """v^T A_e u = int k grad v . grad u for quadratic u, v, k (their interpolants are exact)"""
    exact = sum(_integral_box_tet(_pmul(K, _pmul(_pdiff(V, r), _pdiff(U, r)))) for r in range(3))
    A = pu.element_matrix(BOX_TET, _nodal(K, BOX_TET))
    got = _nodal(V, BOX_TET) @ A @ _nodal(U, BOX_TET)
    assert abs(got - float(exact)) <= 1e-13 * abs(float(exact))


def test_mass_matrix_sums_to_the_volume_and_integrates_quadratics_exactly():
    M = pu.mass_element_matrix(BOX_TET)
    assert abs(M.sum() - 1.0) <= 1e-14  # |e| = 2 * 3 * 1 / 6
    assert np.abs(M - M.T).max() == 0.0
    exact = float(_integral_box_tet(_pmul(U, V)))
    assert abs(_nodal(U, BOX_TET) @ M @ _nodal(V, BOX_TET) - exact) <= 1e-13 * abs(exact)


def test_float64_restatement_agrees_with_its_80_bit_twin():
    rng = np.random.default_rng(5)
    c, k = rng.uniform(-1.0, 1.0, (4, 3)), rng.uniform(0.5, 2.0, 10)
    A, W = pu.element_matrix(c, k), pu.element_matrix(c, k, pu.LD)
    assert W.dtype == pu.LD
    assert float(np.abs(A - W).max()) <= 1e-13 * np.abs(A).max()


@pytest.mark.parametrize("mesh,level", [("cube_6el", 1), ("regular_octahedron_8el", 1), ("cube_6el", 2)])
def test_global_matrix_is_symmetric_and_annihilates_constants(mesh, level):
    v, c = gmgutil.mesh(mesh)
    gidx, ndof = pu.global_numbering(c, level)
    pts = pu.global_points(v, c, gidx, ndof, level)
    # every copy of a shared DoF sits at the same physical position
    for cell, cv in enumerate(np.asarray(c)):
        assert np.abs(pts[gidx[cell]] - pu.dof_points(np.asarray(v)[cv], level)).max() <= 1e-14
    ks = [gmgutil.coefficient(*pu.dof_points(np.asarray(v)[cv], level).T) for cv in np.asarray(c)]
    A, _ = pu.global_matrix(v, c, ks, level)
    scale = abs(A).max()
    assert abs(A - A.T).max() <= 1e-13 * scale
    assert np.abs(A @ np.ones(ndof)).max() <= 1e-12 * scale


def test_prolongation_reproduces_quadratics():
    v, c = gmgutil.mesh("cube_6el")
    (gc, nc), (gf, nf) = pu.global_numbering(c, 1), pu.global_numbering(c, 2)
    P = pu.prolongation(1, gc, nc, gf, nf)
    q = lambda p: p[:, 0] ** 2 - 0.5 * p[:, 1] * p[:, 2] + p[:, 2] + 1.0
    assert np.abs(P @ q(pu.global_points(v, c, gc, nc, 1)) - q(pu.global_points(v, c, gf, nf, 2))).max() <= 1e-13


@pytest.mark.parametrize("level", [2, 3, 4])
def test_known_answer_is_inside_the_bounds_of_the_reference(level):
    """f = M interp( rhs ), Dirichlet data on the whole boundary, direct solve; error = sqrt( sum err^2 / global P2 DoFs )"""
    v, c = gmgutil.mesh("tet_1el")
    err, _ = pu.known_answer(level, tuple(map(tuple, np.asarray(v, dtype=np.float64)[np.asarray(c)[0]])))
    print(f"level {level}: {pu.size(level)} DoFs, error {err:.3e}, bound {pu.KNOWN_BOUNDS[level]:.1e}")
    assert err < pu.KNOWN_BOUNDS[level]
