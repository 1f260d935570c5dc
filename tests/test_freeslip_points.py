"""CPU-only: the shell enumeration the normal projection runs over (hyteg_hip_p1_shell_enumeration) and the points its normal
function is evaluated at (Storage.shell_points).  Nothing here touches a device."""
import numpy as np
import pytest

import freesliputil as fu
import hostutil as hu
from hyteg_amd import capi, host
from oracle import p1_oracle as po


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_shell_enumeration_visits_every_surface_point_once_and_no_inner_point(level):
    N = (1 << level) + 1
    e = fu.enumeration(level)
    assert len(e) == capi.p1_shell_size(level) == 4 * (N * (N + 1) // 2)
    visited = e[e[:, 3] >= 0]
    x, y, z = visited[:, 0], visited[:, 1], visited[:, 2]
    assert ((x >= 0) & (y >= 0) & (z >= 0) & (x + y + z <= N - 1)).all()
    assert ((x * y * z == 0) | (x + y + z == N - 1)).all(), "an inner point is visited"
    pts = [tuple(p) for p in visited[:, :3]]
    assert len(set(pts)) == len(pts), "a point is visited twice"
    surface = {tuple(p) for p in po.cell_coords(level).astype(int) if p[0] * p[1] * p[2] == 0 or p.sum() == N - 1}
    assert set(pts) == surface
    # the slot is that of the macro-primitive the point lies on
    slots = po.slot_of_points(level)
    assert (slots[fu.array_index(level, visited)] == visited[:, 3]).all()
    if level == 4:
        assert len(e) == 612  # more than two workgroups of 256, the last one partly filled


def test_shell_size_of_a_bad_level_is_zero():
    assert capi.p1_shell_size(-1) == 0 and capi.p1_shell_size(12) == 0


def _shell_mesh_radii():
    v, _ = hu.read_msh(hu.MESHES / "spherical_shell_ntan2_3layers.msh")
    r = np.linalg.norm(v, axis=1)
    return r.min(), r.max()


@pytest.mark.parametrize("mesh", ["cube_6el", "spherical_shell_ntan2_3layers"])
@pytest.mark.parametrize("level", [0, 2, 3])
def test_shell_points_are_the_boundary_points_with_identical_copies(mesh, level):
    st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
    pred = fu.cube_vertices_on_boundary if mesh == "cube_6el" else fu.shell_vertices_on_boundary(*_shell_mesh_radii())
    e = fu.enumeration(level)
    idx = fu.array_index(level, e)
    copies = {}
    evaluated = 0
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        got = st.shell_points(i, level)
        assert got.shape == (len(e), 3)
        want = fu.shell_q_points(co, level)
        on_boundary = fu.support_on_boundary(co, level, pred)[idx] & (e[:, 3] >= 0)
        # NaN at the skipped entries and at the points of primitives inside the domain, coordinates everywhere else
        assert (np.isnan(got).all(axis=1) == ~on_boundary).all()
        assert not np.isnan(got[on_boundary]).any()
        # the coordinates of the cell's own micro-vertices, up to the rounding of another summation order
        if on_boundary.any():
            assert np.abs(got[on_boundary] - want[on_boundary]).max() <= 8 * np.finfo(float).eps * np.abs(co).max()
        evaluated += int(on_boundary.sum())
        for q in np.nonzero(on_boundary)[0]:
            copies.setdefault(tuple(np.round(want[q], 9)), []).append(got[q].tobytes())
    assert evaluated > 0
    shared = [c for c in copies.values() if len(c) > 1]
    assert shared, "the mesh has no shared boundary point"
    for c in copies.values():
        assert len(set(c)) == 1, "the copies of a shared point differ in their bits"


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_edge_enumeration_visits_every_surface_edge_dof_once_and_no_other(level):
    n = 1 << level
    e = fu.edge_enumeration(level)
    assert len(e) == capi.p2_edge_shell_size(level) == 12 * (n * (n + 1) // 2)
    visited = e[e[:, 4] >= 0]
    idx = fu.edge_array_index(level, visited)  # KeyError: not an edge DoF of the cell
    assert len(set(idx.tolist())) == len(idx), "an edge DoF is visited twice"
    m2 = fu.edge_midpoints2(level)
    on_surface = (m2.prod(axis=1) == 0) | (m2.sum(axis=1) == 2 * n)  # the midpoint lies on a face of the cell
    assert set(idx.tolist()) == set(np.nonzero(on_surface)[0].tolist())
    # exactly the edge DoFs that the kernels' edge_class puts on a macro-edge or macro-face, with its slot
    classes = po.edge_classes(level)
    assert set(idx.tolist()) == set(np.nonzero(classes < 14)[0].tolist())
    assert (classes[idx] == visited[:, 4]).all()


def test_edge_shell_size_of_a_bad_level_is_zero():
    assert capi.p2_edge_shell_size(-1) == 0 and capi.p2_edge_shell_size(10) == 0


@pytest.mark.parametrize("mesh", ["cube_6el", "spherical_shell_ntan2_3layers"])
@pytest.mark.parametrize("level", [0, 2])
def test_edge_shell_points_are_the_boundary_midpoints_with_identical_copies(mesh, level):
    st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
    pred = fu.cube_vertices_on_boundary if mesh == "cube_6el" else fu.shell_vertices_on_boundary(*_shell_mesh_radii())
    e = fu.edge_enumeration(level)
    visited = e[:, 4] >= 0
    idx = np.zeros(len(e), dtype=np.int64)
    idx[visited] = fu.edge_array_index(level, e[visited])
    copies = {}
    for i in range(st.n_local_cells):
        co = st.local_cell(i)[1]
        got = st.edge_shell_points(i, level)
        assert got.shape == (len(e), 3)
        want = fu.edge_points(co, level)[idx]
        on_boundary = fu.edge_support_on_boundary(co, level, pred)[idx] & visited
        assert (np.isnan(got).all(axis=1) == ~on_boundary).all()
        if on_boundary.any():
            assert np.abs(got[on_boundary] - want[on_boundary]).max() <= 8 * np.finfo(float).eps * np.abs(co).max()
        for q in np.nonzero(on_boundary)[0]:
            copies.setdefault(tuple(np.round(want[q], 9)), []).append(got[q].tobytes())
    assert any(len(c) > 1 for c in copies.values()), "the mesh has no shared boundary edge DoF"
    for c in copies.values():
        assert len(set(c)) == 1, "the copies of a shared edge DoF differ in their bits"
