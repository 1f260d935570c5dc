"""CPU restatement of the variable-coefficient P1 diffusion operator -div( k grad u ) for the tests: a vectorised numpy element
loop over one macro-cell, and a dense global assembly for small levels.

With k a P1 function (linear on a micro-cell) and constant shape-function gradients the element matrix is exact and closed:
    A_e = mean( k at the 4 vertices of e ) * K_e,     K_e[i, j] = |e| grad l_i . grad l_j
(K_e: the P1 Laplace element matrix, pinned by tests/golden/ref_fenics_forms.npz).  Nothing here calls the library under test."""
import functools

import numpy as np

# celldof::macrocell::getMicroVerticesFromMicroCell (volumedofspace/CellDoFIndexing.hpp:155-198), cell types in the order of
# celldof::allCellTypes: WHITE_UP, BLUE_UP, GREEN_UP, WHITE_DOWN, BLUE_DOWN, GREEN_DOWN
MICRO_CELL_VERTS = np.array([
    [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 1]],
    [[1, 0, 0], [0, 1, 0], [1, 0, 1], [0, 0, 1]], [[1, 1, 0], [1, 1, 1], [0, 1, 1], [1, 0, 1]],
    [[1, 0, 1], [0, 1, 1], [0, 0, 1], [0, 1, 0]], [[0, 1, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]]], dtype=np.int64)
MASK_INNER, MASK_SHELL, MASK_ALL = 1 << 14, 0x3FFF, 0x7FFF


def width(level):
    return (1 << level) + 1


def cell_size(level):
    n = width(level)
    return n * (n + 1) * (n + 2) // 6


def cell_index(level, x, y, z):
    """array index of the micro-vertex (x, y, z), vectorised (indexing/MacroCellIndexing.hpp:40-52)"""
    n = width(level)
    w = n - z
    return (n * (n + 1) * (n + 2) - w * (w + 1) * (w + 2)) // 6 + y * w - (y * (y - 1)) // 2 + x


@functools.lru_cache(maxsize=None)
def cell_coords(level):
    """(size, 3) logical (x, y, z) per array entry, in memory order (cached: read-only)"""
    n = width(level)
    out = np.empty((cell_size(level), 3), dtype=np.int32)
    e = 0
    for z in range(n):
        w = n - z
        y, x = np.meshgrid(np.arange(w), np.arange(w), indexing="ij")
        keep = x + y <= w - 1
        m = int(keep.sum())
        out[e:e + m, 0], out[e:e + m, 1], out[e:e + m, 2] = x[keep], y[keep], z
        e += m
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def point_slots(level):
    """per array entry: slot 0..13 of the macro-primitive it lies on (edge0..5, face0..3, vertex0..3), 14 for inner points
    (indexing/MacroCellIndexing.cpp:36-91)"""
    c = cell_coords(level)
    n = width(level)
    f0, f1, f2, f3 = c[:, 2] == 0, c[:, 1] == 0, c[:, 0] == 0, c.sum(axis=1) == n - 1
    cnt = f0.astype(int) + f1 + f2 + f3
    slot = np.full(len(c), 14)
    slot[cnt == 1] = (6 + np.select([f0, f1, f2], [0, 1, 2], 3))[cnt == 1]
    edge = np.select([f0 & f1, f0 & f2, f0 & f3, f1 & f2, f1 & f3], [0, 1, 2, 3, 4], 5)
    slot[cnt == 2] = edge[cnt == 2]
    vert = np.select([f0 & f1 & f2, f0 & f1 & f3, f0 & f2 & f3], [10, 11, 12], 13)
    slot[cnt >= 3] = vert[cnt >= 3]
    if level == 0:  # every point is a macro-vertex
        slot[:] = vert
    slot.setflags(write=False)
    return slot


def point_mask(level, mask):
    """boolean per array entry: its class is selected by the 15-bit mask"""
    return ((mask >> point_slots(level)) & 1).astype(bool)


def cell_points(tet, level):
    """(size, 3) physical coordinates of the micro-vertices in array order"""
    cc = np.asarray(tet, dtype=np.float64).reshape(4, 3)
    ijk = cell_coords(level).astype(np.float64) / float(1 << level)
    return cc[0] + ijk[:, 0:1] * (cc[1] - cc[0]) + ijk[:, 1:2] * (cc[2] - cc[0]) + ijk[:, 2:3] * (cc[3] - cc[0])


@functools.lru_cache(maxsize=None)
def micro_cells(level, t):
    """(cells, 4) array indices of the vertices of every micro-cell of type t inside the macro-cell (cached: read-only)"""
    n = width(level)
    m = cell_coords(level)
    V = MICRO_CELL_VERTS[t]
    # the vertices' coordinates are never negative; the cell lies inside if its vertex with the largest x + y + z does
    m = m[m.sum(axis=1) + int(V.sum(axis=1).max()) <= n - 1].astype(np.int64)
    idx = np.stack([cell_index(level, m[:, 0] + V[j, 0], m[:, 1] + V[j, 1], m[:, 2] + V[j, 2]) for j in range(4)], axis=1).astype(np.int32)
    idx.setflags(write=False)
    return idx


def laplace_element_matrix(c):
    """K[i, j] = |T| grad l_i . grad l_j of the tetrahedron c (4, 3), from its coordinates"""
    c = np.asarray(c, dtype=np.float64).reshape(4, 3)
    J = (c[1:] - c[0]).T
    G = np.linalg.inv(J)  # rows: gradients of l_1 .. l_3
    g = np.vstack([-G.sum(axis=0), G])
    return abs(np.linalg.det(J)) / 6.0 * (g @ g.T)


def micro_element_matrices(tet, level):
    """(6, 4, 4): K_e of the six micro-cell types of the macro-cell `tet` at `level` (constant per type on an affine cell)"""
    cc = np.asarray(tet, dtype=np.float64).reshape(4, 3)
    h = 1.0 / float(1 << level)
    out = np.empty((6, 4, 4))
    for t in range(6):
        v = MICRO_CELL_VERTS[t].astype(np.float64) * h
        out[t] = laplace_element_matrix(cc[0] + v[:, 0:1] * (cc[1] - cc[0]) + v[:, 1:2] * (cc[2] - cc[0]) + v[:, 2:3] * (cc[3] - cc[0]))
    return out


def apply_cell(src, k, tet, level, mask=MASK_ALL):
    """this macro-cell's ( A src ): sum over its micro-cells e of mean_k( e ) K_e src_e, scattered; zero outside the class mask"""
    n = cell_size(level)
    K = micro_element_matrices(tet, level)
    out = np.zeros(n)
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        loc = k[idx].mean(axis=1)[:, None] * (src[idx] @ K[t].T)
        out += np.bincount(idx.ravel(), weights=loc.ravel(), minlength=n)
    if mask != MASK_ALL:
        out[~point_mask(level, mask)] = 0.0
    return out


def diagonal_cell(k, tet, level):
    """this macro-cell's share of the operator's diagonal"""
    n = cell_size(level)
    K = micro_element_matrices(tet, level)
    out = np.zeros(n)
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        loc = k[idx].mean(axis=1)[:, None] * np.diag(K[t])[None, :]
        out += np.bincount(idx.ravel(), weights=loc.ravel(), minlength=n)
    return out


def max_weight(tet, level):
    return float(np.abs(micro_element_matrices(tet, level)).max())


def dense_cell(k, tet, level, mass=False):
    """dense matrix of one macro-cell (rows / columns: its array entries); mass: the P1 mass matrix instead (k ignored)"""
    n = cell_size(level)
    A = np.zeros((n, n))
    K = micro_element_matrices(tet, level)
    cc = np.asarray(tet, dtype=np.float64).reshape(4, 3)
    vol = abs(np.linalg.det((cc[1:] - cc[0]).T)) / 6.0 / float(1 << level) ** 3
    M = vol / 20.0 * (np.ones((4, 4)) + np.eye(4))
    for t in range(6):
        idx = micro_cells(level, t)
        if len(idx) == 0:
            continue
        loc = np.broadcast_to(M, (len(idx), 4, 4)) if mass else k[idx].mean(axis=1)[:, None, None] * K[t][None]
        np.add.at(A, (idx[:, :, None], idx[:, None, :]), loc)
    return A


def global_numbering(mesh_cells, level):
    """per mesh cell: global DoF id of every array entry (shared points get one id), and the number of DoFs.  A point is keyed by
    its non-zero barycentric weights on the mesh vertices, so copies on neighbouring cells coincide."""
    n = width(level) - 1
    ijk = cell_coords(level)
    index, gidx = {}, []
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        g = np.empty(len(ijk), dtype=np.int64)
        for e, (x, y, z) in enumerate(ijk):
            bary = (n - x - y - z, x, y, z)
            key = tuple(sorted((int(cv[a]), int(bary[a])) for a in range(4) if bary[a] > 0))
            if len(key) == 4:
                key = (c, e)
            g[e] = index.setdefault(key, len(index))
        gidx.append(g)
    return gidx, len(index)


def dense_global(vertices, mesh_cells, ks, level):
    """dense global matrix of a mesh: ks[c] is the coefficient's cell array of mesh cell c"""
    gidx, ndof = global_numbering(mesh_cells, level)
    A = np.zeros((ndof, ndof))
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        Ac = dense_cell(ks[c], np.asarray(vertices, dtype=np.float64)[cv], level)
        np.add.at(A, (gidx[c][:, None], gidx[c][None, :]), Ac)
    return A, gidx


# ---- the reference's known answer (tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:103-119) ----
ALPHA, PHI = 2.0, 2.0


def known_k(x, y, z):
    return np.tanh(ALPHA * (x - 0.5)) + 2.0


def known_u(x, y, z):
    return np.sin(PHI * np.pi * x) * np.sinh(np.pi * y)


def known_rhs(x, y, z):
    t0 = np.tanh(ALPHA * (x - 0.5))
    t1 = PHI * ALPHA * (t0 * t0 - 1.0) * np.cos(PHI * np.pi * x)
    t2 = (PHI * PHI - 1.0) * np.pi * (t0 + 2.0) * np.sin(PHI * np.pi * x)
    return np.pi * (t1 + t2) * np.sinh(np.pi * y)


# bounds of the reference test on 3D/tet_1el.msh (lines 175-177)
KNOWN_BOUNDS = {3: 2.5e-3, 4: 7.2e-4, 5: 2.0e-4}


def known_error(u, tet, level):
    """sqrt( err . err / npoints ) with npoints as the reference computes it (lines 144-145): the number of P2 DoFs, which is the P1
    point count of the next level -- NOT the P1 count of this level (normalised by that, level 3 gives 2.6e-3 and misses 2.5e-3)"""
    p = cell_points(tet, level)
    err = u - known_u(p[:, 0], p[:, 1], p[:, 2])
    return float(np.sqrt(err @ err / cell_size(level + 1)))
