"""CPU-only: the restated multigrid cycle on the P2 epsilon operator and the restated block-preconditioned MINRES of the Taylor-Hood
system (tests/p2epsilongmgutil.py: p2epsilonutil.global_matrix per level, p2divkgradutil.prolongation on every component, the cycle,
smoothers and MINRES loop of gmgutil / epsilongmgutil) have the properties a MINRES preconditioner needs, on cube_6el from the lowest
level with a free velocity DoF up to level 2, mu = exp( 3 x )( 1 + y ) (contrast 40), and on the hierarchy of the levels 1-2, the one the GPU
tests run the cycle on (tests/test_gpu_p2_epsilon_gmg.py, tests/test_gpu_p2_epsilon_block_minres.py: no host-layer test exercises P2
functions, their transfer or a coarse CG at level 0, so the GPU comparison starts where that ground is covered)."""
import numpy as np
import pytest

import epsilongmgutil as eg
import p2epsilongmgutil as pg

MESH, HI = "cube_6el", 2
LO = pg.lowest_level(MESH)
LOWEST = [LO, 1]  # the hierarchy from the lowest level with a free DoF, and the one of the GPU tests


def test_the_hierarchy_starts_at_the_lowest_level_with_a_free_velocity_dof():
    """cube_6el: the six tetrahedra share the cube's diagonal, whose midpoint is a free P2 DoF at level 0"""
    assert LO == 0
    h = pg.hierarchy(MESH, LO, HI)
    assert [int(h.levels[l].free.sum()) for l in (0, 1, 2)] == [3, 81, 1029]  # 3 ( 2^( l + 1 ) - 1 )^3


def test_restriction_is_the_transpose_of_the_prolongation():
    h = pg.hierarchy(MESH, LO, HI)  # contains the transfer 1 -> 2 of the GPU tests' hierarchy
    rng = np.random.default_rng(0)
    for l in range(LO, HI):
        u, r = rng.standard_normal(3 * h.levels[l].n), rng.standard_normal(3 * h.levels[l + 1].n)
        assert abs(h.prolongate(u, l) @ r - u @ h.restrict(r, l + 1)) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(r)
        assert np.array_equal(h.restrict(r, l + 1), h.P[l].T @ r)
        n_c, n_f = h.levels[l].n, h.levels[l + 1].n
        for k in range(3):  # component k of the coarse vector reaches component k of the fine one only
            e = np.zeros(3 * n_c)
            e[k * n_c:(k + 1) * n_c] = rng.standard_normal(n_c)
            fine = h.prolongate(e, l).reshape(3, n_f)
            assert np.any(fine[k]) and not np.any(np.delete(fine, k, axis=0))


@pytest.mark.parametrize("lo", LOWEST)
def test_restated_cycle_is_a_symmetric_positive_definite_map(lo):
    """one V( 1, 1 ) Chebyshev( 2 ) cycle from zero applied to the unit vectors of the free DoFs of level 2: what MINRES needs of the
    velocity action.  Asymmetry bound: that of tests/test_epsilon_gmg_restatement.py"""
    h = pg.hierarchy(MESH, lo, HI)
    action = eg.cycle_action(h, eg.smoother(h, "chebyshev", 2), 1, 1)
    free = np.flatnonzero(h.levels[HI].free)
    B = np.zeros((len(free), len(free)))
    for j, g in enumerate(free):
        e = np.zeros(3 * h.levels[HI].n)
        e[g] = 1.0
        z = action(e)
        assert not np.any(z[~h.levels[HI].free])
        B[:, j] = z[free]
    asym = np.abs(B - B.T).max() / np.abs(B).max()
    low = np.linalg.eigvalsh(0.5 * (B + B.T)).min()
    print(f"levels {lo}-{HI}: asymmetry {asym:.3e}, smallest eigenvalue {low:.3e}")
    assert asym <= 1e-13
    assert low > 0.0


@pytest.mark.parametrize("lo", LOWEST)
def test_block_preconditioner_beats_the_pressure_preconditioner_in_the_restated_loop(lo):
    """iterations to 1e-8 of the restated loops on the Taylor-Hood matrix of cube_6el level 2"""
    _, etas = pg.minres(MESH, lo, HI, "block", 3000, rel_tol=1e-8)
    _, etas_p = pg.minres(MESH, lo, HI, "pressure", 3000, rel_tol=1e-8)
    print(f"velocity cycle on the levels {lo}-{HI}: restated MINRES to 1e-8: block {len(etas) - 1}, pressure {len(etas_p) - 1} iterations")
    assert 0 < len(etas) - 1 < len(etas_p) - 1 < 2999
