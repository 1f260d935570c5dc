"""CPU-only: the numpy restatement of the epsilon operator (tests/epsilonutil.py) is pinned by identities that follow from the
weak form  int mu ( grad u + grad u^T ) : grad v,  before anything is compared to it.  A non-axis-aligned tetrahedron (all six
micro-cell types differ), levels 1-3, random mu in [0.5, 50]."""
import functools

import numpy as np
import pytest

import divkgradutil as dk
import epsilonutil as eu
from conftest import SKEW_TET

LEVELS = [1, 2, 3]


@functools.lru_cache(maxsize=None)
def case(level):
    rng = np.random.default_rng(500 + level)
    mu = rng.uniform(0.5, 50.0, dk.cell_size(level))
    A = eu.dense_cell(mu, SKEW_TET, level)
    mu.setflags(write=False)
    A.setflags(write=False)
    return mu, A


@pytest.mark.parametrize("level", LEVELS)
def test_trace_of_the_blocks_is_four_times_divkgrad(level):
    """sum_i A^{ii} = 4 * ( the div-k-grad matrix with k = mu ): sum_i ( g_a . g_b + g_a[i] g_b[i] ) = 4 g_a . g_b"""
    mu, A = case(level)
    n = dk.cell_size(level)
    trace = sum(A[i * n:(i + 1) * n, i * n:(i + 1) * n] for i in range(3))
    want = 4.0 * dk.dense_cell(mu, SKEW_TET, level)
    assert np.abs(trace - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("level", LEVELS)
def test_dense_matrix_is_symmetric(level):
    _, A = case(level)
    assert np.abs(A - A.T).max() <= 1e-14 * np.abs(A).max()


@pytest.mark.parametrize("level", LEVELS)
def test_rigid_motions_are_in_the_kernel_of_inner_rows(level):
    """a + b x X for the six unit ( a, b ): zero at the inner rows (levels 2, 3), to 1e-12 * max mu * max |element entry| * max |u|;
    level 1 has no inner row: the sum over all rows of the cell is zero there as well (no boundary terms in the weak form)"""
    mu, A = case(level)
    n = dk.cell_size(level)
    X = dk.cell_points(SKEW_TET, level)
    inner = np.tile(dk.point_mask(level, dk.MASK_INNER), 3)
    for k in range(6):
        a, b = np.zeros(3), np.zeros(3)
        (a if k < 3 else b)[k % 3] = 1.0
        u = (a[None, :] + np.cross(b[None, :], X)).T.reshape(3 * n)
        bound = 1e-12 * mu.max() * eu.max_weight(SKEW_TET, level) * np.abs(u).max()
        r = A @ u
        assert np.abs(r[inner]).max(initial=0.0) <= bound
        # every row: eps( rigid motion ) = 0 on every micro-cell
        assert np.abs(r).max() <= bound
        assert np.abs(eu.apply_cell(u.reshape(3, n), mu, SKEW_TET, level)).max() <= bound


@pytest.mark.parametrize("level", LEVELS)
def test_energy_of_linear_fields(level):
    """u = ( x, 0, 0 ): u^T A u = 2 int mu;  u = ( y, 0, 0 ): int mu  -- pins the factor 2"""
    mu, A = case(level)
    n = dk.cell_size(level)
    X = dk.cell_points(SKEW_TET, level)
    integral = eu.integral_of_mu(mu, SKEW_TET, level)
    for axis, factor in ((0, 2.0), (1, 1.0)):
        u = np.zeros(3 * n)
        u[:n] = X[:, axis]
        energy = u @ (A @ u)
        assert abs(energy - factor * integral) <= 1e-13 * factor * integral
        v = eu.apply_cell(u.reshape(3, n), mu, SKEW_TET, level).reshape(3 * n)
        assert abs(u @ v - factor * integral) <= 1e-13 * factor * integral


@pytest.mark.parametrize("level", LEVELS)
def test_constant_viscosity_scales_the_operator(level):
    n = dk.cell_size(level)
    c = 7.25
    A1, Ac = eu.dense_cell(np.ones(n), SKEW_TET, level), eu.dense_cell(np.full(n, c), SKEW_TET, level)
    assert np.abs(Ac - c * A1).max() <= 1e-14 * np.abs(Ac).max()


@pytest.mark.parametrize("level", LEVELS)
def test_element_loop_and_diagonal_agree_with_the_dense_matrix(level):
    mu, A = case(level)
    n = dk.cell_size(level)
    u = np.random.default_rng(600 + level).uniform(-1.0, 1.0, (3, n))
    want = (A @ u.reshape(3 * n)).reshape(3, n)
    assert np.abs(eu.apply_cell(u, mu, SKEW_TET, level) - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(eu.diagonal_cell(mu, SKEW_TET, level).reshape(3 * n) - np.diag(A)).max() <= 1e-13 * np.diag(A).max()


def test_cuboid_mesh_is_the_unit_cube_in_six_tetrahedra():
    v, c = eu.cuboid_mesh()
    assert v.shape == (8, 3) and c.shape == (6, 4)
    vol = [abs(np.linalg.det((v[t[1:]] - v[t[0]]).T)) / 6.0 for t in c]
    assert np.allclose(vol, 1.0 / 6.0) and abs(sum(vol) - 1.0) <= 1e-15
    assert sorted(set(c.ravel())) == list(range(8))
