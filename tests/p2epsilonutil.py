"""CPU restatement of the variable-viscosity P2 epsilon operator -div( 2 mu eps(u) ), eps(u) = ( grad u + grad u^T ) / 2, with a P2
viscosity, and of the Taylor-Hood Stokes operator built on it, for the tests.  Everything sits on top of tests/p2divkgradutil.py: the
universal tensor U[m, i, j, a, b] = int_e phi_m d phi_i / d l_a d phi_j / d l_b / |e| (exact rational integration), the layout of a
macro-cell's DoF vector and the global numbering by physical position.

Weak form  int mu ( grad u + grad u^T ) : grad v.  For the test function phi_i e_p and the trial function phi_j e_q
    A_e^{pq}[i, j] = int_e mu ( delta_pq grad phi_j . grad phi_i + d_p phi_j d_q phi_i )
                   = |e| sum_m mu_m sum_ab U[m, i, j, a, b] ( delta_pq g_a . g_b + g_a[q] g_b[p] ),
mu the P2 interpolant of its ten values on e: a degree-4 integrand, integrated exactly.  Vectors of three components are component-major:
( u entries, v entries, w entries ) of the DoF vector of p2divkgradutil.  The pressure of the Taylor-Hood matrix lives on the vertex
DoFs; the mixed blocks  - int q d_k u  are integrated with the same rational machinery.  Nothing here calls the library under test."""
import functools
import itertools
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import divkgradutil as dk
import epsilonutil as eu
import p2divkgradutil as pu

MASK_INNER, MASK_SHELL, MASK_ALL = pu.MASK_INNER, pu.MASK_SHELL, pu.MASK_ALL


def weights(g):
    """(3, 3, 4, 4): W[p, q, a, b] = delta_pq g_a . g_b + g_a[q] g_b[p] from the (4, 3) barycentric gradients"""
    gg = g @ g.T
    W = np.empty((3, 3, 4, 4), dtype=g.dtype)
    for p, q in itertools.product(range(3), range(3)):
        W[p, q] = (gg if p == q else 0) + np.outer(g[:, q], g[:, p])
    return W


def element_blocks(c, mu, dtype=np.float64):
    """(3, 3, 10, 10): A_e^{pq}[i, j] of the tetrahedron c (4, 3) with the ten viscosity values mu"""
    g, vol = pu.gradients(c, dtype)
    U, _ = pu.universal(dtype)
    return vol * np.einsum("m,mijab,pqab->pqij", np.asarray(mu, dtype=dtype), U, weights(g))


def element_matrix(c, mu, dtype=np.float64):
    """(30, 30), component-major"""
    return element_blocks(c, mu, dtype).transpose(0, 2, 1, 3).reshape(30, 30)


def micro_cell(tet, level, t, dtype=np.float64):
    cc = np.asarray(tet, dtype=dtype).reshape(4, 3)
    v = dk.MICRO_CELL_VERTS[t].astype(dtype) / dtype(1 << level)
    return cc[0] + v[:, 0:1] * (cc[1] - cc[0]) + v[:, 1:2] * (cc[2] - cc[0]) + v[:, 2:3] * (cc[3] - cc[0])


def type_tensors(tet, level, dtype=np.float64):
    """(6, 3, 3, 10, 10, 10): T[t, p, q, m, i, j] = int_e phi_m ( delta_pq grad phi_j . grad phi_i + d_p phi_j d_q phi_i ) of the six
    micro-cell types of the macro-cell"""
    U, _ = pu.universal(dtype)
    out = np.empty((6, 3, 3, 10, 10, 10), dtype=dtype)
    for t in range(6):
        g, vol = pu.gradients(micro_cell(tet, level, t, dtype), dtype)
        out[t] = vol * np.einsum("mijab,pqab->pqmij", U, weights(g))
    return out


def cell_matrix(mu, tet, level, dtype=np.float64):
    """sparse (3 n, 3 n) matrix of one macro-cell on its component-major DoF vector: the sum over its micro-cells of A_e( mu_e )"""
    n = pu.size(level)
    T = type_tensors(tet, level, dtype)
    mu = np.asarray(mu, dtype=dtype)
    rows, cols, vals = [], [], []
    for t in range(6):
        idx = pu.micro_cell_dofs(level, t)
        if len(idx) == 0:
            continue
        loc = np.einsum("em,pqmij->epqij", mu[idx], T[t])  # (cells, 3, 3, 10, 10)
        r = idx[:, None, None, :, None] + n * np.arange(3)[None, :, None, None, None]
        c = idx[:, None, None, None, :] + n * np.arange(3)[None, None, :, None, None]
        rows.append(np.broadcast_to(r, loc.shape).ravel()), cols.append(np.broadcast_to(c, loc.shape).ravel()), vals.append(loc.ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * n, 3 * n))


def dof_masks(level, masks, kinds=0xFF):
    """(3, n) boolean: the DoFs the per-component class masks (one mask, or three) and the kind mask select"""
    masks = list(masks) if isinstance(masks, (tuple, list)) else [masks] * 3
    return np.stack([pu.dof_mask(level, m, kinds) for m in masks])


def max_entry(tet, level):
    """max | T |: with max mu it bounds the entries of every A_e from above, up to the factor 10"""
    return float(np.abs(type_tensors(tet, level)).max())


def global_matrix(vertices, mesh_cells, mus, level, dtype=np.float64):
    """sparse (3 N, 3 N) global matrix of a mesh, component-major over the numbering of p2divkgradutil.global_numbering; mus[c]: the
    viscosity on the DoF vector of mesh cell c.  Returns (A, gidx, N)."""
    gidx, ndof = pu.global_numbering(mesh_cells, level)
    A = sp.csr_matrix((3 * ndof, 3 * ndof), dtype=dtype)
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        Ac = cell_matrix(mus[c], np.asarray(vertices, dtype=np.float64)[cv], level, dtype).tocoo()
        g3 = np.concatenate([gidx[c] + k * ndof for k in range(3)])
        A = A + sp.csr_matrix((Ac.data, (g3[Ac.row], g3[Ac.col])), shape=(3 * ndof, 3 * ndof))
    return A, gidx, ndof


# ---- the mixed blocks of the Taylor-Hood operator ----
@functools.lru_cache(maxsize=None)
def _divergence_fractions():
    """D[i, j, b] = int_e l_i d phi_j / d l_b / |e|, i a vertex (P1 shape function l_i), j a P2 shape function"""
    phi = pu.shape_functions()
    D = np.empty((4, 10, 4), dtype=object)
    for i, j, b in itertools.product(range(4), range(10), range(4)):
        d = pu._diff(phi[j], b)
        D[i, j, b] = pu._integral(pu._mul({pu._unit(i): Fraction(1)}, d)) if d else Fraction(0)
    return D


@functools.lru_cache(maxsize=None)
def divergence_constants(dtype=np.float64):
    return pu._as(dtype, _divergence_fractions())


def pressure_numbering(gidx, level):
    """the pressure DoFs are the vertex DoFs: per mesh cell the pressure ids of its vertex array, and their number"""
    nv = pu.vertex_size(level)
    ids = np.unique(np.concatenate([g[:nv] for g in gidx]))
    lookup = {int(v): k for k, v in enumerate(ids)}
    return [np.array([lookup[int(v)] for v in g[:nv]], dtype=np.int64) for g in gidx], len(ids)


def divergence_matrix(vertices, mesh_cells, level, gidx, ndof, dtype=np.float64):
    """sparse (Np, 3 N): B[i, ( k, j )] = - int l_i d_k phi_j (P2ToP1 div blocks); its transpose is the divT block.  Returns (B, pidx, Np)"""
    pidx, npr = pressure_numbering(gidx, level)
    D = divergence_constants(dtype)
    B = sp.csr_matrix((npr, 3 * ndof), dtype=dtype)
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        tet = np.asarray(vertices, dtype=np.float64)[cv]
        rows, cols, vals = [], [], []
        for t in range(6):
            idx = pu.micro_cell_dofs(level, t)
            if len(idx) == 0:
                continue
            g, vol = pu.gradients(micro_cell(tet, level, t, dtype), dtype)
            loc = -vol * np.einsum("ijb,bk->kij", D, g)  # (3, 4, 10)
            r = pidx[c][idx[:, :4]][:, None, :, None]
            col = gidx[c][idx][:, None, None, :] + ndof * np.arange(3)[None, :, None, None]
            shape = (len(idx), 3, 4, 10)
            rows.append(np.broadcast_to(r, shape).ravel()), cols.append(np.broadcast_to(col, shape).ravel())
            vals.append(np.broadcast_to(loc[None], shape).ravel())
        B = B + sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(npr, 3 * ndof))
    return B, pidx, npr


def lumped_pressure_mass(vertices, mesh_cells, level, pidx, npr):
    """row sums of the global P1 mass matrix: every micro-cell gives |e| / 4 to each of its vertices (what P1LumpedInvMassOperator inverts)"""
    out = np.zeros(npr)
    for c, cv in enumerate(np.asarray(mesh_cells, dtype=np.int64)):
        tet = np.asarray(vertices, dtype=np.float64)[cv]
        for t in range(6):
            idx = pu.micro_cell_dofs(level, t)
            if len(idx):
                np.add.at(out, pidx[c][idx[:, :4]].ravel(), pu.gradients(micro_cell(tet, level, t))[1] / 4.0)
    return out


def taylor_hood_matrix(vertices, mesh_cells, mus, level, dtype=np.float64):
    """sparse (3 N + Np, 3 N + Np): [[ A_eps, B^T ], [ B, 0 ]], the matrix of P2P1StokesEpsilonOperator, ( u, v, w, p ).
    Returns (S, gidx, N, pidx, Np)"""
    A, gidx, N = global_matrix(vertices, mesh_cells, mus, level, dtype)
    B, pidx, npr = divergence_matrix(vertices, mesh_cells, level, gidx, N, dtype)
    return sp.bmat([[A, B.T], [B, None]], format="csr"), gidx, N, pidx, npr


# ---- the reference's known answer (tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:73-91, P2 3-D case :366-412) ----
KNOWN_BOUNDS = {2: (2.2e-1, 1.8e+1), 3: (3.0e-2, 1.9)}


def boundary_dofs(vertices, mesh_cells, level, gidx, ndof):
    """global mask of the P2 DoFs on the boundary of the unit cube of cuboid_mesh()"""
    pts = pu.global_points(vertices, mesh_cells, gidx, ndof, level)
    return (np.abs(pts) < 1e-12).any(axis=1) | (np.abs(pts - 1.0) < 1e-12).any(axis=1)


@functools.lru_cache(maxsize=None)
def known_answer(level):
    """direct sparse solve of the reference's P2-P1 case: MeshInfo::meshCuboid( 0, 1, 1 x 1 x 1 ), mu = 1, velocity Dirichlet on the whole
    boundary, f = M interp( rhs ) per component, zero pressure right-hand side.  Pressure DoFs with no free velocity DoF in their support
    (the cube corners that belong to one tetrahedron) have an empty row: they are dropped and stay at zero, as in a MINRES run from a
    zero pressure.  The constant the system leaves open is fixed as that run fixes it: its iterates lie in M^-1 times a Krylov space
    orthogonal to the null vector, M the lumped pressure mass, so the mass-weighted sum of the kept pressures is zero.  Then projectMean
    over ALL pressure DoFs.  Returns (errors u, v, w, p as sqrt( err . err / DoFs ); the solution (3, N), (Np,); the numberings)"""
    vertices, cells = eu.cuboid_mesh()
    mus = [np.ones(pu.size(level)) for _ in cells]
    S, gidx, N, pidx, npr = taylor_hood_matrix(vertices, cells, mus, level)
    M = pu.global_matrix(vertices, cells, None, level, mass=True)[0]
    pts = pu.global_points(vertices, cells, gidx, N, level)
    x, y, z = pts.T
    exact = np.stack([eu.known_u(x, y, z), eu.known_v(x, y, z), eu.known_w(x, y, z)])
    f = np.stack([M @ fn(x, y, z) for fn in (eu.known_rhs_u, eu.known_rhs_v, eu.known_rhs_w)])
    bnd = boundary_dofs(vertices, cells, level, gidx, N)
    start = np.concatenate([np.where(bnd, exact, 0.0).reshape(3 * N), np.zeros(npr)])
    rhs = np.concatenate([f.reshape(3 * N), np.zeros(npr)]) - S @ start
    free_v = np.tile(~bnd, 3)
    B = S[3 * N:, :3 * N]
    kept = np.asarray(abs(B[:, free_v]).sum(axis=1)).ravel() > 0.0
    free = np.concatenate([free_v, kept])
    lumped = lumped_pressure_mass(vertices, cells, level, pidx, npr)
    nfree = int(free.sum())
    c = np.zeros(nfree)
    c[int(free_v.sum()):] = lumped[kept]
    K = sp.bmat([[S[free][:, free], sp.csr_matrix(c[:, None])], [sp.csr_matrix(c[None, :]), None]], format="csc")
    sol = spla.spsolve(K, np.concatenate([rhs[free], [0.0]]))
    full = start.copy()
    full[free] += sol[:nfree]
    u, p = full[:3 * N].reshape(3, N), full[3 * N:]
    p = p - p.mean()
    pp = np.zeros(npr)
    for c_, cv in enumerate(np.asarray(cells, dtype=np.int64)):
        q = pu.dof_points(np.asarray(vertices, dtype=np.float64)[cv], level)[:pu.vertex_size(level)]
        pp[pidx[c_]] = eu.known_p(q[:, 0], q[:, 1], q[:, 2])
    pp -= pp.mean()
    errors = [float(np.sqrt(((u[k] - exact[k]) ** 2).sum() / N)) for k in range(3)] + [float(np.sqrt(((p - pp) ** 2).sum() / npr))]
    return errors, u, p, (gidx, N, pidx, npr), int((~kept).sum())
