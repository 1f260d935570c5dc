"""CPU restatement of the variable-coefficient P2 diffusion operator -div( k grad u ) with a P2 coefficient, for the tests: exact
element matrices from the monomial formula, sparse per-cell and global matrices, the P2 mass matrix, the quadratic prolongation
between two levels and the reference's known answer (tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp, runAllTestsP2).

On a micro-cell e with barycentric functions l_0 .. l_3 the ten shape functions are written out as polynomials in l (vertex: 2 l_a^2 - l_a,
edge: 4 l_a l_b, FEniCS order: vertices 0-3, edges (2,3) (1,3) (1,2) (0,3) (0,2) (0,1)), differentiated term by term, multiplied, and
integrated monomial by monomial with  int_e l^alpha = 6 |e| alpha! / ( |alpha| + 3 )!  in rational arithmetic:
    U[m, i, j, a, b] = int_e phi_m  d phi_i / d l_a  d phi_j / d l_b  / |e|            (universal)
    A_e[i, j]        = |e| sum_m k_m sum_ab U[m, i, j, a, b] grad l_a . grad l_b
Every function takes a dtype: numpy.longdouble gives the 80-bit twin that measures the rounding of the float64 restatement.
A macro-cell's DoFs are one vector: its vertex array followed by its edge array (blocks X, Y, Z, XY, XZ, YZ of tet( 2^level ) entries, then
XYZ of tet( 2^level - 1 )).  Nothing here calls the library under test."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import divkgradutil as dk

LD = np.longdouble
MASK_INNER, MASK_SHELL, MASK_ALL = dk.MASK_INNER, dk.MASK_SHELL, dk.MASK_ALL
EDGE_PAIRS = [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]  # local DoFs 4 .. 9
# end points of an edge DoF relative to its logical index, kinds 1 .. 7 = X, Y, Z, XY, XZ, YZ, XYZ (edgedofspace/EdgeDoFIndexing.hpp:89-210)
EDGE_ENDS = np.array([[[0, 0, 0], [1, 0, 0]], [[0, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0]],
                      [[1, 0, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1]], [[0, 1, 0], [1, 0, 1]]], dtype=np.int64)


# ---- polynomials in l_0 .. l_3: { exponent tuple: Fraction } ----
def _mul(p, q):
    out = {}
    for (ea, ca), (eb, cb) in itertools.product(p.items(), q.items()):
        e = tuple(x + y for x, y in zip(ea, eb))
        out[e] = out.get(e, 0) + ca * cb
    return out


def _diff(p, a):
    out = {}
    for e, c in p.items():
        if e[a]:
            d = list(e)
            d[a] -= 1
            out[tuple(d)] = out.get(tuple(d), 0) + c * e[a]
    return out


def _integral(p):
    """int_e p / |e|"""
    return sum(c * Fraction(6 * math.prod(math.factorial(x) for x in e), math.factorial(sum(e) + 3)) for e, c in p.items())


def _unit(a, power=1):
    return tuple(power if r == a else 0 for r in range(4))


def shape_functions():
    phi = [{_unit(a, 2): Fraction(2), _unit(a): Fraction(-1)} for a in range(4)]
    phi += [{tuple(int(r in (a, b)) for r in range(4)): Fraction(4)} for a, b in EDGE_PAIRS]
    return phi


@functools.lru_cache(maxsize=None)
def _universal_fractions():
    phi = shape_functions()
    d = [[_diff(p, a) for a in range(4)] for p in phi]
    U = np.empty((10, 10, 10, 4, 4), dtype=object)
    for i, j, a, b in itertools.product(range(10), range(10), range(4), range(4)):
        g = _mul(d[i][a], d[j][b])
        for m in range(10):
            U[m, i, j, a, b] = _integral(_mul(phi[m], g)) if g else Fraction(0)
    M = np.empty((10, 10), dtype=object)
    for i, j in itertools.product(range(10), range(10)):
        M[i, j] = _integral(_mul(phi[i], phi[j]))
    return U, M


def _as(dtype, fractions):
    flat = [dtype(f.numerator) / dtype(f.denominator) for f in fractions.ravel()]
    return np.array(flat, dtype=dtype).reshape(fractions.shape)


@functools.lru_cache(maxsize=None)
def universal(dtype=np.float64):
    """U[m, i, j, a, b] and the mass constants M[i, j] = int phi_i phi_j / |e|"""
    U, M = _universal_fractions()
    return _as(dtype, U), _as(dtype, M)


def gradients(c, dtype=np.float64):
    """(4, 3) gradients of the barycentric functions of the tetrahedron c and its volume"""
    c = np.asarray(c, dtype=dtype).reshape(4, 3)
    J = (c[1:] - c[0]).T
    det = (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
           + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))
    cof = np.array([[J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1], J[0, 2] * J[2, 1] - J[0, 1] * J[2, 2], J[0, 1] * J[1, 2] - J[0, 2] * J[1, 1]],
                    [J[1, 2] * J[2, 0] - J[1, 0] * J[2, 2], J[0, 0] * J[2, 2] - J[0, 2] * J[2, 0], J[0, 2] * J[1, 0] - J[0, 0] * J[1, 2]],
                    [J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0], J[0, 1] * J[2, 0] - J[0, 0] * J[2, 1], J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]]],
                   dtype=dtype) / det
    return np.vstack([-cof.sum(axis=0), cof]), abs(det) / dtype(6)


def element_matrix(c, k, dtype=np.float64):
    """A_e (10, 10) of the tetrahedron c (4, 3) with the ten coefficient values k"""
    g, vol = gradients(c, dtype)
    U, _ = universal(dtype)
    return vol * np.einsum("m,mijab,ab->ij", np.asarray(k, dtype=dtype), U, g @ g.T)


def mass_element_matrix(c, dtype=np.float64):
    return gradients(c, dtype)[1] * universal(dtype)[1]


def type_tensors(tet, level, dtype=np.float64):
    """(6, 10, 10, 10): T_t[m, i, j] = int_e phi_m grad phi_i . grad phi_j for the six micro-cell types of the macro-cell, and |e|"""
    cc = np.asarray(tet, dtype=dtype).reshape(4, 3)
    h = dtype(1) / dtype(1 << level)
    U, _ = universal(dtype)
    out = np.empty((6, 10, 10, 10), dtype=dtype)
    for t in range(6):
        v = dk.MICRO_CELL_VERTS[t].astype(dtype) * h
        g, vol = gradients(cc[0] + v[:, 0:1] * (cc[1] - cc[0]) + v[:, 1:2] * (cc[2] - cc[0]) + v[:, 2:3] * (cc[3] - cc[0]), dtype)
        out[t] = vol * np.einsum("mijab,ab->mij", U, g @ g.T)
    return out, vol


# ---- layout of a macro-cell's DoF vector ----
def tet(w):
    return w * (w + 1) * (w + 2) // 6 if w > 0 else 0


def tet_index(W, x, y, z):
    w = W - z
    return (W * (W + 1) * (W + 2) - w * (w + 1) * (w + 2)) // 6 + y * w - (y * (y - 1)) // 2 + x


def vertex_size(level):
    return tet((1 << level) + 1)


def edge_size(level):
    n = 1 << level
    return 6 * tet(n) + tet(n - 1)


def size(level):
    return vertex_size(level) + edge_size(level)


def kind_width(level, kind):
    n = 1 << level
    return n + 1 if kind == 0 else (n - 1 if kind == 7 else n)


def kind_start(level, kind):
    return 0 if kind == 0 else vertex_size(level) + (kind - 1) * tet(1 << level)


def _tet_coords(W):
    if W <= 0:
        return np.zeros((0, 3), dtype=np.int64)
    return np.array([(x, y, z) for z in range(W) for y in range(W - z) for x in range(W - z - y)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def dof_table(level):
    """per DoF of the cell vector: kind (0 vertex, 1 .. 7 edge orientation), logical index (3), DOUBLED integer position (3),
    and point class (0 .. 13 macro-edge / -face / -vertex, 14 inner: the class of the macro-primitive that holds all its end points)"""
    N = (1 << level) + 1
    kinds, idx, pos2, cls = [], [], [], []
    for kind in range(8):
        p = _tet_coords(kind_width(level, kind))
        ends = [p] if kind == 0 else [p + EDGE_ENDS[kind - 1][0], p + EDGE_ENDS[kind - 1][1]]
        f = [np.all([e[:, 2] == 0 for e in ends], axis=0), np.all([e[:, 1] == 0 for e in ends], axis=0),
             np.all([e[:, 0] == 0 for e in ends], axis=0), np.all([e.sum(axis=1) == N - 1 for e in ends], axis=0)]
        f0, f1, f2, f3 = f
        cnt = sum(x.astype(int) for x in f)
        c = np.full(len(p), 14)
        c[cnt == 1] = (6 + np.select([f0, f1, f2], [0, 1, 2], 3))[cnt == 1]
        c[cnt == 2] = np.select([f0 & f1, f0 & f2, f0 & f3, f1 & f2, f1 & f3], [0, 1, 2, 3, 4], 5)[cnt == 2]
        c[cnt >= 3] = np.select([f0 & f1 & f2, f0 & f1 & f3, f0 & f2 & f3], [10, 11, 12], 13)[cnt >= 3]
        kinds.append(np.full(len(p), kind)), idx.append(p), cls.append(c)
        pos2.append(2 * p if kind == 0 else ends[0] + ends[1])
    out = tuple(np.concatenate(a) for a in (kinds, idx, pos2, cls))
    assert len(out[0]) == size(level)
    for a in out:
        a.setflags(write=False)
    return out


def dof_mask(level, mask=MASK_ALL, kinds=0xFF):
    kind, _, _, cls = dof_table(level)
    return (((mask >> cls) & 1) & ((kinds >> kind) & 1)).astype(bool)


def dof_points(tet_, level, dtype=np.float64):
    """(size, 3) physical positions of the DoFs (edge DoFs: the midpoints of their micro-edges)"""
    cc = np.asarray(tet_, dtype=dtype).reshape(4, 3)
    p = dof_table(level)[2].astype(dtype) / dtype(2 << level)
    return cc[0] + p[:, 0:1] * (cc[1] - cc[0]) + p[:, 1:2] * (cc[2] - cc[0]) + p[:, 2:3] * (cc[3] - cc[0])


def _edge_dof(level, a, b):
    """index in the cell vector of the edge DoF between the micro-vertices a and b ((cells, 3) each, b - a the same for all cells)"""
    d = b[0] - a[0]
    for kind in range(1, 8):
        e0, e1 = EDGE_ENDS[kind - 1]
        if np.array_equal(d, e1 - e0) or np.array_equal(-d, e1 - e0):
            p = (a if np.array_equal(d, e1 - e0) else b) - e0
            return kind_start(level, kind) + tet_index(kind_width(level, kind), p[:, 0], p[:, 1], p[:, 2])
    raise AssertionError("not a micro-edge")


@functools.lru_cache(maxsize=None)
def micro_cell_dofs(level, t):
    """(cells, 10) indices in the cell vector of the ten DoFs of every micro-cell of type t, FEniCS order"""
    N = (1 << level) + 1
    V = dk.MICRO_CELL_VERTS[t]
    m = _tet_coords(N)
    m = m[m.sum(axis=1) + int(V.sum(axis=1).max()) <= N - 1]
    if len(m) == 0:
        return np.zeros((0, 10), dtype=np.int64)
    v = [m + V[j] for j in range(4)]
    cols = [tet_index(N, p[:, 0], p[:, 1], p[:, 2]) for p in v] + [_edge_dof(level, v[a], v[b]) for a, b in EDGE_PAIRS]
    out = np.stack(cols, axis=1)
    out.setflags(write=False)
    return out


# ---- matrices ----
def cell_matrix(k, tet_, level, dtype=np.float64, mass=False):
    """sparse matrix of one macro-cell on its DoF vector: sum over its micro-cells of A_e( k_e ) (mass: of |e| M)"""
    n = size(level)
    T, vol = type_tensors(tet_, level, dtype)
    k = np.asarray(k, dtype=dtype)
    rows, cols, vals = [], [], []
    for t in range(6):
        idx = micro_cell_dofs(level, t)
        if len(idx) == 0:
            continue
        loc = np.broadcast_to(vol * universal(dtype)[1], (len(idx), 10, 10)) if mass else np.einsum("em,mij->eij", k[idx], T[t])
        rows.append(np.broadcast_to(idx[:, :, None], loc.shape).ravel()), cols.append(np.broadcast_to(idx[:, None, :], loc.shape).ravel())
        vals.append(loc.ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def apply_cell(src, k, tet_, level, mask=MASK_ALL, kinds=0xFF, dtype=np.float64):
    out = cell_matrix(k, tet_, level, dtype) @ np.asarray(src, dtype=dtype)
    out[~dof_mask(level, mask, kinds)] = 0
    return out


def diagonal_cell(k, tet_, level, dtype=np.float64):
    return cell_matrix(k, tet_, level, dtype).diagonal()


def max_entry(tet_, level):
    """max | int_e phi_m grad phi_i . grad phi_j |: with max k it bounds the entries of every A_e from above, up to the factor 10"""
    return float(np.abs(type_tensors(tet_, level)[0]).max())


def global_numbering(mesh_cells, level):
    """per mesh cell: global id of every entry of its DoF vector, and the number of DoFs.  A DoF is keyed by its physical position,
    written as doubled integer barycentric weights on the mesh vertices, so copies on neighbouring cells coincide"""
    n2 = 2 << level
    pos2 = dof_table(level)[2]
    index, gidx = {}, []
    for cv in np.asarray(mesh_cells, dtype=np.int64):
        g = np.empty(len(pos2), dtype=np.int64)
        for e, (x, y, z) in enumerate(pos2):
            bary = (n2 - x - y - z, x, y, z)
            key = tuple(sorted((int(cv[a]), int(bary[a])) for a in range(4) if bary[a] > 0))
            g[e] = index.setdefault(key, len(index))
        gidx.append(g)
    return gidx, len(index)


def global_matrix(vertices, mesh_cells, ks, level, dtype=np.float64, mass=False):
    """sparse global matrix of a mesh; ks[c]: the coefficient on the DoF vector of mesh cell c"""
    gidx, ndof = global_numbering(mesh_cells, level)
    A = sp.csr_matrix((ndof, ndof), dtype=dtype)
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        Ac = cell_matrix(None if mass else ks[c], np.asarray(vertices, dtype=np.float64)[cv], level, dtype, mass).tocoo()
        A = A + sp.csr_matrix((Ac.data, (gidx[c][Ac.row], gidx[c][Ac.col])), shape=(ndof, ndof))
    return A, gidx


def global_points(vertices, mesh_cells, gidx, ndof, level):
    out = np.zeros((ndof, 3))
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        out[gidx[c]] = dof_points(np.asarray(vertices, dtype=np.float64)[cv], level)
    return out


def to_global(gidx, ndof, arrays, dtype=np.float64):
    out = np.zeros(ndof, dtype=dtype)
    for g, a in zip(gidx, arrays):
        out[g] = a
    return out


# ---- quadratic prolongation: the coarse P2 basis evaluated at the fine DoFs ----
def basis_at(lam):
    """(points, 10) values of the ten shape functions at barycentric coordinates lam (points, 4)"""
    cols = [lam[:, a] * (2 * lam[:, a] - 1) for a in range(4)] + [4 * lam[:, a] * lam[:, b] for a, b in EDGE_PAIRS]
    return np.stack(cols, axis=1)


def prolongation(coarse_level, gidx_c, ndof_c, gidx_f, ndof_f):
    """(ndof_f, ndof_c): row of a fine DoF = the coarse shape functions of a coarse micro-cell that contains it, evaluated there.
    A coarse micro-cell with the vertices m + V_a holds the 35 points sum_a L_a ( m + V_a ), L_a >= 0 integers with sum 4, of the
    DOUBLED fine integer lattice, every one a fine DoF; its barycentric coordinates are L / 4.  The rows a shared DoF gets from
    several micro-cells coincide (the trace of a P2 function on a face is unique): checked, then one of them is kept."""
    fine = coarse_level + 1
    q = dof_table(fine)[2]
    side = (4 << coarse_level) + 1
    lookup = np.full(side ** 3, -1, dtype=np.int64)
    lookup[(q[:, 2] * side + q[:, 1]) * side + q[:, 0]] = np.arange(len(q))
    L = np.array([l for l in itertools.product(range(5), repeat=4) if sum(l) == 4], dtype=np.int64)
    W = basis_at(L / 4.0)  # (35, 10)
    N = (1 << coarse_level) + 1
    ii, jj, ww = [], [], []
    for gc, gf in zip(gidx_c, gidx_f):
        for t in range(6):
            V = dk.MICRO_CELL_VERTS[t]
            m = _tet_coords(N)
            m = m[m.sum(axis=1) + int(V.sum(axis=1).max()) <= N - 1]
            if len(m) == 0:
                continue
            pts = np.einsum("pa,car->cpr", L, m[:, None, :] + V[None, :, :])  # (cells, 35, 3)
            f = lookup[(pts[..., 2] * side + pts[..., 1]) * side + pts[..., 0]]
            assert (f >= 0).all()
            dofs = micro_cell_dofs(coarse_level, t)
            ii.append(np.broadcast_to(gf[f][:, :, None], (len(m), 35, 10)).ravel())
            jj.append(np.broadcast_to(gc[dofs][:, None, :], (len(m), 35, 10)).ravel())
            ww.append(np.broadcast_to(W[None], (len(m), 35, 10)).ravel())
    i, j, w = np.concatenate(ii), np.concatenate(jj), np.concatenate(ww)
    keep = w != 0
    i, j, w = i[keep], j[keep], w[keep]
    S = sp.csr_matrix((w, (i, j)), shape=(ndof_f, ndof_c))
    S2 = sp.csr_matrix((w * w, (i, j)), shape=(ndof_f, ndof_c))
    C = sp.csr_matrix((np.ones_like(w), (i, j)), shape=(ndof_f, ndof_c))
    for X in (S, S2, C):
        X.sum_duplicates(), X.sort_indices()
    assert np.array_equal(S.indices, C.indices) and np.allclose(S2.data * C.data, S.data ** 2, rtol=1e-14, atol=0)
    return sp.csr_matrix((S.data / C.data, S.indices, S.indptr), shape=S.shape)


# ---- the reference's known answer (ElementwiseDivKGradCGConvergenceTest.cpp:103-119, runAllTestsP2 :192-221) ----
known_k, known_u, known_rhs = dk.known_k, dk.known_u, dk.known_rhs
KNOWN_BOUNDS = {2: 4.5e-3, 3: 4.6e-4, 4: 3.8e-5}
UNIT_TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def interpolate(fn, tet_, level):
    p = dof_points(tet_, level)
    return fn(p[:, 0], p[:, 1], p[:, 2])


def _as_tet(tet_):
    return UNIT_TET if tet_ is None else np.asarray(tet_, dtype=np.float64).reshape(4, 3)


@functools.lru_cache(maxsize=None)
def known_answer(level, tet_=None):
    """direct solve of the known-answer problem on a one-cell mesh (tet_: a hashable tuple of its 4 x 3 coordinates, default the unit
    tetrahedron): f = M interp( rhs ), Dirichlet data u on the whole boundary.  Returns (error as the reference computes it, solution
    on the DoF vector)"""
    t = _as_tet(tet_)
    k = interpolate(known_k, t, level)
    A = cell_matrix(k, t, level)
    M = cell_matrix(None, t, level, mass=True)
    u_exact = interpolate(known_u, t, level)
    free = dof_table(level)[3] == 14
    x = np.where(free, 0.0, u_exact)
    rhs = (M @ interpolate(known_rhs, t, level) - A @ x)[free]
    x[free] = spla.spsolve(sp.csc_matrix(A[free][:, free]), rhs)
    return known_error(x, level, tet_), x


def known_error(u, level, tet_=None):
    """sqrt( sum err^2 / number of global P2 DoFs ), as the reference computes it"""
    err = u - interpolate(known_u, _as_tet(tet_), level)
    return float(np.sqrt(err @ err / size(level)))
