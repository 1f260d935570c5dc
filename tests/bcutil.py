"""Test helpers for per-primitive boundary conditions: the outflow cube of the reference's
P1Stokes3DMinResConvergenceTest (cube_24el, everything on the boundary flag 1, the inside of the face z = 1 flag 2) and the
per-point truth of it, computed from coordinates alone."""
import numpy as np

from hostutil import MESHES, cell_points
from hyteg_amd import host

CUBE = MESHES / "cube_24el.msh"
EPS = 1e-9


def on_outflow(x, y, z):
    """strictly inside the face z = 1 of the unit cube"""
    return abs(z - 1.0) < EPS and EPS < x < 1.0 - EPS and EPS < y < 1.0 - EPS


def outflow_cube(how="centroid", rank=0, nranks=1, mesh=CUBE):
    """the storage with flag 2 on the macro-vertex, -edges and -faces of z = 1 that do not touch its rim"""
    st = host.Storage.from_gmsh(mesh, rank, nranks)
    st.set_mesh_boundary_flags_on_boundary(1, 0, True)
    if how == "centroid":
        st.set_mesh_boundary_flags_by_centroid_location(2, on_outflow)
    else:
        for dim in range(3):
            for i in range(st.n_primitives(dim)):
                p = st.primitive(dim, i)
                if on_outflow(*p.coordinates.mean(axis=0)):
                    st.set_mesh_boundary_flag(dim, i, 2)
    return st


def flags_of(st):
    return [[st.primitive(dim, i).flag for i in range(st.n_primitives(dim))] for dim in range(3)]


def point_types(points):
    """per point (n, 3) of the unit cube: host.NeumannBoundary strictly inside z = 1, host.DirichletBoundary elsewhere on the
    surface, host.Inner inside"""
    P = np.asarray(points, dtype=np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    surface = (np.minimum(P, 1.0 - P) < EPS).any(axis=1)
    neumann = (np.abs(z - 1.0) < EPS) & (x > EPS) & (x < 1.0 - EPS) & (y > EPS) & (y < 1.0 - EPS)
    t = np.full(len(P), host.Inner)
    t[surface] = host.DirichletBoundary
    t[neumann] = host.NeumannBoundary
    return t


def truth(st, level, flag):
    """per local cell: boolean per array entry, selected by `flag` according to the coordinates"""
    return [(point_types(cell_points(st.local_cell(i)[1], level)) & flag) != 0 for i in range(st.n_local_cells)]


def point_key(p):
    return tuple(np.round(p, 9))
