"""CPU restatement of the variable-viscosity epsilon operator -div( 2 mu eps(u) ), eps(u) = ( grad u + grad u^T ) / 2, for the
tests: a vectorised numpy element loop over one macro-cell and dense assemblies for small levels.  Nothing here calls the library
under test.

Weak form  int 2 mu eps(u) : eps(v) = int mu ( grad u + grad u^T ) : grad v.  With mu a P1 function (linear on a micro-cell e) and
constant barycentric gradients g_a the block for test component i and trial component j is exact and closed:
    A_e^{ij}[a][b] = mean( mu at the 4 vertices of e ) * |e| * ( delta_ij g_a . g_b + g_a[j] g_b[i] ).
Layout of the vectors and matrices of three components: component-major, ( u entries, v entries, w entries ).  The div / divT /
PSPG / mass element matrices of the Stokes matrix are those of oracle/p1_oracle (pinned by tests/test_oracle_pins.py)."""
import numpy as np

from divkgradutil import (MASK_ALL, MASK_INNER, MASK_SHELL, MICRO_CELL_VERTS, cell_coords, cell_points, cell_size, global_numbering,  # noqa: F401
                          micro_cells, point_mask)


def _micro_cell(tet, level, t):
    cc = np.asarray(tet, dtype=np.float64).reshape(4, 3)
    v = MICRO_CELL_VERTS[t].astype(np.float64) / float(1 << level)
    return cc[0] + v[:, 0:1] * (cc[1] - cc[0]) + v[:, 1:2] * (cc[2] - cc[0]) + v[:, 2:3] * (cc[3] - cc[0])


def gradients(c):
    """(4, 3) gradients of the barycentric functions of the tetrahedron c (4, 3), and its volume"""
    c = np.asarray(c, dtype=np.float64).reshape(4, 3)
    J = (c[1:] - c[0]).T
    G = np.linalg.inv(J)  # rows: gradients of l_1 .. l_3
    return np.vstack([-G.sum(axis=0), G]), abs(np.linalg.det(J)) / 6.0


def element_blocks(tet, level):
    """(6, 3, 3, 4, 4): B[t, i, j, a, b] = |e| ( delta_ij g_a . g_b + g_a[j] g_b[i] ) of the six micro-cell types (mu = 1)"""
    out = np.empty((6, 3, 3, 4, 4))
    for t in range(6):
        g, vol = gradients(_micro_cell(tet, level, t))
        gg = g @ g.T
        for i in range(3):
            for j in range(3):
                out[t, i, j] = vol * ((gg if i == j else 0.0) + np.outer(g[:, j], g[:, i]))
    return out


def micro_volumes(tet, level):
    return np.array([gradients(_micro_cell(tet, level, t))[1] for t in range(6)])


def max_weight(tet, level):
    return float(np.abs(element_blocks(tet, level)).max())


def apply_cell(srcs, mu, tet, level, mask=MASK_ALL):
    """this macro-cell's ( A src ), (3, n): sum over its micro-cells e of mean_mu( e ) sum_j B_e^{ij} src_j, scattered; zero outside
    the class mask"""
    n = cell_size(level)
    B = element_blocks(tet, level)
    srcs = np.asarray(srcs, dtype=np.float64).reshape(3, n)
    out = np.zeros((3, n))
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        m = mu[idx].mean(axis=1)[:, None]
        # one product per type: rows ( i, a ), columns ( j, b ) of the 12 x 12 element matrix
        E = B[t].transpose(0, 2, 1, 3).reshape(12, 12)
        loc = (np.concatenate([srcs[j][idx] for j in range(3)], axis=1) @ E.T) * m
        for i in range(3):
            out[i] += np.bincount(idx.ravel(), weights=loc[:, 4 * i:4 * i + 4].ravel(), minlength=n)
    if mask != MASK_ALL:
        out[:, ~point_mask(level, mask)] = 0.0
    return out


def diagonal_cell(mu, tet, level):
    """(3, n): this macro-cell's share of the diagonals of the diagonal blocks A^{ii}"""
    n = cell_size(level)
    B = element_blocks(tet, level)
    out = np.zeros((3, n))
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        m = mu[idx].mean(axis=1)[:, None]
        for i in range(3):
            loc = m * np.diag(B[t, i, i])[None, :]
            out[i] += np.bincount(idx.ravel(), weights=loc.ravel(), minlength=n)
    return out


def integral_of_mu(mu, tet, level):
    """int mu over the macro-cell: sum over the micro-cells of mean mu times volume (exact for P1 mu)"""
    vol = micro_volumes(tet, level)
    return float(sum(vol[t] * mu[micro_cells(level, t)].mean(axis=1).sum() for t in range(6) if len(micro_cells(level, t))))


def dense_cell(mu, tet, level):
    """(3 n, 3 n) dense matrix of one macro-cell, component-major"""
    n = cell_size(level)
    A = np.zeros((3, 3, n, n))
    B = element_blocks(tet, level)
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        m = mu[idx].mean(axis=1)[:, None, None]
        for i in range(3):
            for j in range(3):
                np.add.at(A[i, j], (idx[:, :, None], idx[:, None, :]), m * B[t, i, j][None])
    return A.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)


def dense_global(vertices, mesh_cells, mus, level):
    """(3 N, 3 N) dense global matrix of the 3-component block, component-major over the global numbering of
    divkgradutil.global_numbering; mus[c]: the viscosity's cell array of mesh cell c.  Returns (A, gidx, N)."""
    gidx, ndof = global_numbering(mesh_cells, level)
    n = cell_size(level)
    A = np.zeros((3 * ndof, 3 * ndof))
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        Ac = dense_cell(mus[c], np.asarray(vertices, dtype=np.float64)[cv], level)
        g3 = np.concatenate([gidx[c] + k * ndof for k in range(3)])
        assert len(g3) == 3 * n
        np.add.at(A, (g3[:, None], g3[None, :]), Ac)
    return A, gidx, ndof


def _scalar_global(vertices, mesh_cells, level, gidx, ndof, form):
    """dense global matrix of a constant-coefficient P1 form of oracle/p1_oracle (test rows, trial columns)"""
    from oracle import p1_oracle as po

    M = np.zeros((ndof, ndof))
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        tet = np.asarray(vertices, dtype=np.float64)[cv]
        for t in range(6):
            idx = micro_cells(level, t)
            if len(idx) == 0:
                continue
            E = po.element_matrix(_micro_cell(tet, level, t), form)
            g = gidx[c][idx]
            np.add.at(M, (g[:, :, None], g[:, None, :]), np.broadcast_to(E, (len(idx), 4, 4)))
    return M


def dense_stokes_global(vertices, mesh_cells, mus, level):
    """(4 N, 4 N): the matrix of P1P1ElementwiseAffineEpsilonStokesOperator, [[ A_eps, divT ], [ div, pspg ]], component-major
    ( u, v, w, p ).  Returns (S, gidx, N)."""
    from oracle import p1_oracle as po

    A, gidx, N = dense_global(vertices, mesh_cells, mus, level)
    S = np.zeros((4 * N, 4 * N))
    S[:3 * N, :3 * N] = A
    for k in range(3):
        S[k * N:(k + 1) * N, 3 * N:] = _scalar_global(vertices, mesh_cells, level, gidx, N, po.FORM_DIVT_X + k)
        S[3 * N:, k * N:(k + 1) * N] = _scalar_global(vertices, mesh_cells, level, gidx, N, po.FORM_DIV_X + k)
    S[3 * N:, 3 * N:] = _scalar_global(vertices, mesh_cells, level, gidx, N, po.FORM_PSPG)
    return S, gidx, N


def lumped_mass_global(vertices, mesh_cells, level, gidx, ndof):
    """row sums of the global P1 mass matrix (what P1LumpedInvMassOperator inverts)"""
    from oracle import p1_oracle as po

    return _scalar_global(vertices, mesh_cells, level, gidx, ndof, po.FORM_MASS).sum(axis=1)


def to_global(arrays, gidx, ndof):
    """cell arrays of one scalar function -> global vector (copies of a shared point agree)"""
    out = np.zeros(ndof)
    for a, g in zip(arrays, gidx):
        out[g] = a
    return out


def to_cells(vec, gidx):
    return [np.ascontiguousarray(vec[g]) for g in gidx]


# ---- the reference's 3-D known answer (tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:73-91) ----
def known_u(x, y, z):
    return -4.0 * np.cos(4.0 * z)


def known_v(x, y, z):
    return 8.0 * np.cos(8.0 * x)


def known_w(x, y, z):
    return -2.0 * np.cos(2.0 * y)


def known_p(x, y, z):
    return np.sin(4.0 * x) * np.sin(8.0 * y) * np.sin(2.0 * z)


def known_rhs_u(x, y, z):
    return 4.0 * np.sin(8.0 * y) * np.sin(2.0 * z) * np.cos(4.0 * x) - 64.0 * np.cos(4.0 * z)


def known_rhs_v(x, y, z):
    return 8.0 * np.sin(4.0 * x) * np.sin(2.0 * z) * np.cos(8.0 * y) + 512.0 * np.cos(8.0 * x)


def known_rhs_w(x, y, z):
    return 2.0 * np.sin(4.0 * x) * np.sin(8.0 * y) * np.cos(2.0 * z) - 8.0 * np.cos(2.0 * y)


# bounds of the reference test (lines 302-309 of the same file: level -> (each velocity component, pressure))
KNOWN_BOUNDS = {3: (5.9e-1, 2.4e+1), 4: (2.2e-1, 8.7)}


def cuboid_mesh():
    """the 8 vertices and 6 tetrahedra of MeshInfo::meshCuboid( (0,0,0), (1,1,1), 1, 1, 1 ): the tables of
    src/hyteg/mesh/MeshGenCuboid.cpp:71-115 (vertex id = ( iz * 2 + iy ) * 2 + ix; tNode: the six tetrahedra in the standard
    hexahedron numbering, offset: that numbering's corners), cells in the order of the reference's std::map (lexicographic)"""
    t_node = [(4, 5, 7, 3), (0, 3, 1, 4), (4, 1, 5, 3), (5, 6, 7, 2), (1, 3, 2, 5), (7, 2, 3, 5)]
    offset = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    vertices = np.array([(ix, iy, iz) for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)], dtype=np.float64)
    cells = sorted(tuple((offset[m][2] * 2 + offset[m][1]) * 2 + offset[m][0] for m in tet) for tet in t_node)
    return vertices, np.array(cells, dtype=np.int32)
