"""CPU-only: the numpy restatement of the P2 epsilon operator -div( 2 mu eps(u) ) with a P2 viscosity (tests/p2epsilonutil.py) is pinned
before anything is compared with it: algebraic identities of the element blocks, the recorded FEniCS matrices, an independent
numerical quadrature, the reference's four-point sampling where both are exact, and the reference's known answer
(tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp, P2 3-D case) through a direct sparse solve."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import gmgutil
import p2divkgradutil as pu
import p2epsilonutil as pe
from ref_golden import ref_fenics

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_fenics_forms.npz"


def random_case(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (4, 3)), rng.uniform(0.5, 2.0, 10), rng


def nodes(c):
    return np.array([c[a] for a in range(4)] + [(c[a] + c[b]) / 2.0 for a, b in pu.EDGE_PAIRS])


@pytest.mark.parametrize("seed", range(3))
def test_block_transposition_symmetry_and_zero_row_sums(seed):
    c, mu, _ = random_case(seed)
    A = pe.element_blocks(c, mu)
    scale = np.abs(A).max()
    for p in range(3):
        for q in range(3):
            assert np.abs(A[q, p] - A[p, q].T).max() <= 1e-14 * scale
            assert np.abs(A[p, q].sum(axis=1)).max() <= 1e-13 * scale  # a constant trial component has no gradient
    E = pe.element_matrix(c, mu)
    assert np.abs(E - E.T).max() <= 1e-14 * scale


@pytest.mark.parametrize("seed", range(3))
def test_diagonal_blocks_sum_to_four_times_div_k_grad(seed):
    """sum_i ( grad phi_j . grad phi_i + d_i phi_j d_i phi_i ) = 4 grad phi_j . grad phi_i"""
    c, mu, _ = random_case(10 + seed)
    A = pe.element_blocks(c, mu)
    D = pu.element_matrix(c, mu)
    assert np.abs(A[0, 0] + A[1, 1] + A[2, 2] - 4.0 * D).max() <= 1e-14 * np.abs(D).max() * 4.0


def test_unit_viscosity_trace_is_four_times_the_recorded_fenics_laplace_matrices():
    with np.load(GOLDEN) as g:
        coords = g["ref_p2_tet_diffusion__coords"]
    assert len(coords) >= 1
    ref = ref_fenics()
    for c in coords:
        out = np.zeros(100)
        cc = np.ascontiguousarray(c, dtype=np.float64)
        ref.ref_p2_tet_diffusion(out.ctypes.data_as(C.POINTER(C.c_double)), cc.ctypes.data_as(C.POINTER(C.c_double)))
        A = pe.element_blocks(c.reshape(4, 3), np.ones(10))
        assert np.abs(A[0, 0] + A[1, 1] + A[2, 2] - 4.0 * out.reshape(10, 10)).max() <= 1e-13 * 4.0 * np.abs(out).max()


def test_divergence_blocks_are_the_recorded_fenics_matrices():
    """the mixed blocks of the Taylor-Hood restatement: - int l_i d_k phi_j against p2_to_p1_tet_div_tet_cell_integral_k"""
    with np.load(GOLDEN) as g:
        coords, ks, outs = g["ref_p2_to_p1_tet_div__coords"], g["ref_p2_to_p1_tet_div__k"], g["ref_p2_to_p1_tet_div__out"]
    assert len(coords) >= 3
    D = pe.divergence_constants()
    for c, k, out in zip(coords, ks, outs):
        grad, vol = pu.gradients(c.reshape(4, 3))
        B = -vol * np.einsum("ijb,b->ij", D, grad[:, int(k)])
        assert np.abs(B - out.reshape(4, 10)).max() <= 1e-13 * np.abs(out).max()


@pytest.mark.parametrize("seed", range(2))
def test_energy_of_a_uniaxial_stretch_is_twice_the_integral_of_mu(seed):
    """u = ( x, 0, 0 ): ( grad u + grad u^T ) : grad u = 2, so u^T A_e u = 2 int_e mu = 2 . 1^T M mu"""
    c, mu, _ = random_case(20 + seed)
    u = np.zeros((3, 10))
    u[0] = nodes(c)[:, 0]
    E = pe.element_matrix(c, mu)
    energy = u.reshape(30) @ E @ u.reshape(30)
    want = 2.0 * np.ones(10) @ pu.mass_element_matrix(c) @ mu
    assert abs(energy - want) <= 1e-13 * abs(want)


@pytest.mark.parametrize("mesh,level", [("cube_6el", 1), ("regular_octahedron_8el", 1)])
def test_rigid_motions_are_in_the_kernel_of_the_global_matrix(mesh, level):
    """three translations and three infinitesimal rotations (linear fields: their P2 interpolants are exact), variable viscosity"""
    v, c = gmgutil.mesh(mesh)
    mus = [np.exp(3.0 * p[:, 0]) * (1.0 + p[:, 1]) for p in (pu.dof_points(np.asarray(v, dtype=np.float64)[cv], level) for cv in np.asarray(c))]
    A, gidx, N = pe.global_matrix(v, c, mus, level)
    scale = abs(A).max()
    assert abs(A - A.T).max() <= 1e-13 * scale
    x = pu.global_points(v, c, gidx, N, level)
    zero, one = np.zeros(N), np.ones(N)
    motions = [(one, zero, zero), (zero, one, zero), (zero, zero, one), (zero, -x[:, 2], x[:, 1]), (x[:, 2], zero, -x[:, 0]),
               (-x[:, 1], x[:, 0], zero)]
    for m in motions:
        assert np.abs(A @ np.concatenate(m)).max() <= 1e-12 * scale
    # and a field that strains is not
    assert np.abs(A @ np.concatenate((x[:, 0], zero, zero))).max() > 1e-3 * scale


def _shape_gradients(lam, g):
    """(10, 3) gradients of the ten shape functions at the barycentric point lam"""
    rows = [(4.0 * lam[a] - 1.0) * g[a] for a in range(4)] + [4.0 * (lam[a] * g[b] + lam[b] * g[a]) for a, b in pu.EDGE_PAIRS]
    return np.array(rows)


def _duffy_rule(n):
    """tensor Gauss-Legendre rule on the collapsed unit tetrahedron: exact for total degree 2 n - 3; barycentric points and weights that
    sum to one"""
    t, w = np.polynomial.legendre.leggauss(n)
    t, w = 0.5 * (t + 1.0), 0.5 * w
    pts, wts = [], []
    for a, wa in zip(t, w):
        for b, wb in zip(t, w):
            for c, wc in zip(t, w):
                x, y, z = a, b * (1.0 - a), c * (1.0 - a) * (1.0 - b)
                pts.append((1.0 - x - y - z, x, y, z)), wts.append(6.0 * wa * wb * wc * (1.0 - a) ** 2 * (1.0 - b))
    return np.array(pts), np.array(wts)


@pytest.mark.parametrize("seed", range(2))
def test_independent_numerical_quadrature(seed):
    """a collapsed 5 x 5 x 5 Gauss rule (exact to degree 7) on the integrand written out pointwise: the shape functions' gradients from
    the barycentric formulas, mu from the shape functions' values; no use of the universal tensor"""
    c, mu, _ = random_case(30 + seed)
    g, vol = pu.gradients(c)
    pts, wts = _duffy_rule(5)
    assert abs(wts.sum() - 1.0) <= 1e-14
    A = np.zeros((3, 3, 10, 10))
    for lam, w in zip(pts, wts):
        G = _shape_gradients(lam, g)
        m = float(pu.basis_at(lam[None, :])[0] @ mu)
        gg = G @ G.T
        for p in range(3):
            for q in range(3):
                A[p, q] += w * vol * m * ((gg if p == q else 0.0) + np.outer(G[:, q], G[:, p]))
    want = pe.element_blocks(c, mu)
    assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("seed", range(2))
def test_linear_viscosity_and_linear_field_agree_with_the_four_point_sampling(seed):
    """the reference's affine epsilon forms sample the viscosity at the four points of a degree-2 rule.  With mu linear on the cell and u
    linear the integrand mu ( grad u + grad u^T ) : grad phi_i has degree 2 and the rule is exact: the two operators coincide"""
    c, _, rng = random_case(40 + seed)
    x = nodes(c)
    mu = 2.0 + x @ rng.uniform(0.1, 0.3, 3)
    grad_u = rng.uniform(-1.0, 1.0, (3, 3))  # d_r u^p at [p, r]
    u = (x @ grad_u.T).T + rng.uniform(-1.0, 1.0, 3)[:, None]
    g, vol = pu.gradients(c)
    a, b = 0.5854101966249685, 0.1381966011250105
    sym = grad_u + grad_u.T
    want = np.zeros((3, 10))
    for k in range(4):
        lam = np.full(4, b)
        lam[k] = a
        G = _shape_gradients(lam, g)
        want += 0.25 * vol * float(lam @ mu[:4]) * (sym @ G.T)
    got = (pe.element_matrix(c, mu) @ u.reshape(30)).reshape(3, 10)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_float64_restatement_agrees_with_its_80_bit_twin():
    c, mu, _ = random_case(50)
    A, W = pe.element_blocks(c, mu), pe.element_blocks(c, mu, pu.LD)
    assert W.dtype == pu.LD
    assert float(np.abs(A - W).max()) <= 1e-13 * np.abs(A).max()


def test_cell_matrix_is_the_sum_of_its_element_matrices():
    """level 0: one micro-cell; level 1 against a plain loop over the micro-cells"""
    c, _, rng = random_case(60)
    if np.linalg.det((c[1:] - c[0]).T) < 0:
        c = c[[0, 2, 1, 3]]
    mu = rng.uniform(0.5, 2.0, pu.size(1))
    A = pe.cell_matrix(mu, c, 1).toarray()
    n = pu.size(1)
    want = np.zeros((3 * n, 3 * n))
    for t in range(6):
        for dofs in pu.micro_cell_dofs(1, t):
            verts = pu.dof_points(c, 1)[dofs[:4]]
            ix = np.concatenate([dofs + k * n for k in range(3)])
            want[np.ix_(ix, ix)] += pe.element_matrix(verts, mu[dofs])
    assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("level", [2, 3])
def test_known_answer_is_inside_the_bounds_of_the_reference(level):
    """MeshInfo::meshCuboid( 0, 1, 1 x 1 x 1 ), mu = 1, Dirichlet velocity on the whole boundary, errors sqrt( err . err / DoFs ) after
    projectMean.  Two pressure DoFs (cube corners that belong to a single tetrahedron) have no free velocity DoF in their support.
    Solved here: level 2: u 1.241e-1 v 2.129e-1 w 4.719e-2 p 1.783e+1; level 3: u 1.474e-2 v 2.951e-2 w 6.938e-3 p 1.873"""
    errors, u, p, (gidx, N, pidx, npr), dropped = pe.known_answer(level)
    bound_v, bound_p = pe.KNOWN_BOUNDS[level]
    print(f"level {level}: {3 * N + npr} unknowns, errors u {errors[0]:.3e} v {errors[1]:.3e} w {errors[2]:.3e} (bound {bound_v:.1e}), "
          f"p {errors[3]:.3e} (bound {bound_p:.1e}); {dropped} pressure DoFs without a free velocity DoF")
    assert dropped == 2
    assert all(0.0 < e < bound_v for e in errors[:3])
    assert 0.0 < errors[3] < bound_p
    recorded = {2: (1.241e-1, 2.129e-1, 4.719e-2, 1.783e+1), 3: (1.474e-2, 2.951e-2, 6.938e-3, 1.873)}[level]
    assert all(abs(e - r) <= 1e-3 * r for e, r in zip(errors, recorded))  # the four digits written down
