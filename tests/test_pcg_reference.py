"""CPU-only: the numpy restatement of the preconditioned CG loop (tests/pcgutil.py) that the GPU tests of the preconditioned
CGSolver compare against, pinned against textbook PCG with an explicit symmetric Gauss-Seidel matrix; the (a)symmetry of the
reference's forward + backward sweep schedule on one and on several macro-cells; and the symbols the feature exports."""
import ctypes
import functools

import numpy as np
import pytest

import hostutil as hu
import pcgutil

NEW_HIP = ["hyteg_hip_p1_cg_update_cells"]
NEW_HOST = ["hyteg_host_cg_create_preconditioned", "hyteg_host_p2_cg_create_preconditioned", "hyteg_host_cg_set_use_fused_update",
            "hyteg_host_smoother_create", "hyteg_host_p2_smoother_create", "hyteg_host_p2_cg_iterations"]


@functools.lru_cache(maxsize=None)
def _glob(mesh, level):
    v, c = hu.read_msh(hu.MESHES / f"{mesh}.msh")
    return hu.GlobalSweepOracle(v, c, level)


def test_the_restated_loop_is_textbook_pcg_with_the_symmetric_gauss_seidel_matrix():
    """tet_1el, level 3: every free point is an inner point of the one macro-cell, swept in array order, so forward + backward
    Gauss-Seidel from zero is M^-1 with M = (D + L) D^-1 (D + U) of the inner block.  Three iterations, iterate by iterate."""
    glob = _glob("tet_1el", 3)
    free = pcgutil.free_points(glob)
    assert free.sum() == 35  # the inner points of a level-3 cell
    K = pcgutil.dense_matrix(glob)
    Kii = K[np.ix_(free, free)]  # global numbers of a single cell ascend in array order: this is the sweep's order
    D, L, U = np.diag(np.diag(Kii)), np.tril(Kii, -1), np.triu(Kii, 1)
    M = (D + L) @ np.linalg.inv(D) @ (D + U)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    rng = np.random.default_rng(1)
    b, x0 = rng.standard_normal(glob.ndof), rng.standard_normal(glob.ndof)  # non-zero start and non-zero Dirichlet values
    got, its, iterates = pcgutil.pcg(glob.matvec, pcgutil.sweep_preconditioner(glob), x0, b, free, 3)
    assert its == 3 and len(iterates) == 3
    # textbook PCG on the inner block (e.g. Saad, Iterative Methods for Sparse Linear Systems, algorithm 9.1)
    rhs = b[free] - K[np.ix_(free, ~free)] @ x0[~free]
    x = x0[free].copy()
    r = rhs - Kii @ x
    z = np.linalg.solve(M, r)
    p = z.copy()
    for k in range(3):
        Ap = Kii @ p
        alpha = (r @ z) / (p @ Ap)
        x = x + alpha * p
        r_new = r - alpha * Ap
        z_new = np.linalg.solve(M, r_new)
        p = z_new + ((r_new @ z_new) / (r @ z)) * p
        r, z = r_new, z_new
        assert np.abs(iterates[k][free] - x).max() <= 1e-13 * np.abs(x).max(), k
        assert np.array_equal(iterates[k][~free], x0[~free])
    assert np.abs(x - x0[free]).max() > 1e-3 * np.abs(x).max()  # the iterations moved x


@pytest.mark.parametrize("mesh,level,symmetric", [("tet_1el", 3, True), ("tet_1el", 4, True), ("cube_6el", 2, False),
                                                  ("regular_octahedron_8el", 2, False), ("cube_6el", 3, False)])
def test_forward_then_backward_sweep_is_symmetric_on_one_macro_cell_only(mesh, level, symmetric):
    """The backward sweep refreshes the communicated values before every primitive class, the forward sweep does not
    (P1Operator.hpp:373-412): on several macro-cells the pair is not a symmetric operator.  With the random pair of default_rng(1):
    0 and 0 on tet_1el levels 3, 4 (other seeds: up to 4e-17); 1.8e-3, 2.7e-4, 1.0e-5 on cube_6el 2, regular_octahedron_8el 2,
    cube_6el 3 (another random pair gave 5.6e-4, 7.8e-5, 3.5e-5: the same orders of magnitude)."""
    a = pcgutil.asymmetry(_glob(mesh, level))
    print(f"{mesh} level {level}: asymmetry {a:.2e}")
    if symmetric:
        assert a <= 1e-14
    else:
        assert a > 1e-6


@pytest.mark.parametrize("mesh,level", [("cube_6el", 2), ("tet_1el", 3)])
def test_the_sweep_preconditioner_saves_iterations(mesh, level):
    """the two problems the GPU tests solve: iterations to a relative residual of 1e-10 from a zero start"""
    glob = _glob(mesh, level)
    free = pcgutil.free_points(glob)
    b = np.random.default_rng(1).standard_normal(glob.ndof)
    counts = []
    for precond in (pcgutil.identity_preconditioner, pcgutil.sweep_preconditioner(glob)):
        x, its, _ = pcgutil.pcg(glob.matvec, precond, np.zeros(glob.ndof), b, free, 200, 1e-10)
        r = (b - glob.matvec(x))[free]
        assert np.linalg.norm(r) <= 10 * 1e-10 * np.linalg.norm(b[free])
        counts.append(its)
    print(f"{mesh} level {level}: plain {counts[0]}, preconditioned {counts[1]}")
    assert counts[1] < counts[0]


def test_both_libraries_export_the_new_symbols():
    from hyteg_amd import capi, host

    for path, names, mod in ((capi.lib_path(), NEW_HIP, capi), (host.lib_path(), NEW_HOST, host)):
        raw = ctypes.CDLL(str(path))
        for name in names:
            assert hasattr(raw, name), f"{name} is not exported by {path.name}"
            assert name in mod.SIGNATURES, f"{name} has no ctypes binding"
    assert (host.SYMMETRIC_GAUSS_SEIDEL, host.SYMMETRIC_SOR) == (5, 6)


def test_cg_update_cells_validates_its_arguments_on_the_host():
    """EINVAL before any GPU work (made-up addresses: nothing is dereferenced on the host)"""
    from hyteg_amd import capi

    ALL = 0x7FFF
    X, R, P, AP, S, W = [4096], [8192], [12288], [16384], 20480, 24576
    many = capi.HYTEG_HIP_MAX_BATCH + 1
    for match, args in (("level out of range", (X, R, P, AP, 0.5, -1, [ALL], [ALL], S, W)),
                        ("level out of range", (X, R, P, AP, 0.5, 12, [ALL], [ALL], S, W)),
                        ("ncells", ([], [], [], [], 0.5, 3, [], [], S, W)),
                        ("ncells", (X * many, R * many, P * many, AP * many, 0.5, 3, [ALL] * many, [ALL] * many, S, W)),
                        ("null pointer", (None, R, P, AP, 0.5, 3, [ALL], [ALL], S, W)),
                        ("null pointer", (X, R, P, AP, 0.5, 3, [ALL], None, S, W)),
                        ("null pointer", (X, R, P, AP, 0.5, 3, [ALL], [ALL], None, W)),
                        ("null pointer", (X, R, P, AP, 0.5, 3, [ALL], [ALL], S, None)),
                        ("null array", (X, R, [0], AP, 0.5, 3, [ALL], [ALL], S, W)),
                        ("alias", (X, X, P, AP, 0.5, 3, [ALL], [ALL], S, W)),
                        ("alias", (X, R, X, AP, 0.5, 3, [ALL], [ALL], S, W)),
                        ("alias", (X, R, P, X, 0.5, 3, [ALL], [ALL], S, W)),
                        ("alias", (X, R, R, AP, 0.5, 3, [ALL], [ALL], S, W)),
                        ("alias", (X, R, P, R, 0.5, 3, [ALL], [ALL], S, W))):
        with pytest.raises(capi.HytegHipError, match=match):
            capi.p1_cg_update_cells(*args)
