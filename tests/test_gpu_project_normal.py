"""P1ProjectNormalOperator on the GPU (hyteg_hip_p1_project_normal_cells through the host layer) against the numpy restatement
of the reference's point loops (tests/freesliputil.py): parity entry by entry, untouched entries bit for bit, identical copies
of shared points, the known answers of tests/hyteg/freeslip/ProjectNormalTest.cpp, and a recorded launch."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from freesliputil import CENTRE, make_storage, oblique, radial_about  # noqa: E402


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host


def flag_part_of_the_boundary(st, part):
    """mesh flag 3 (free-slip under create0123BC) on: "all" the boundary; one boundary "face"; that face and its "rim".
    Returns the vertex-id sets of the flagged primitives."""
    if part == "all":
        st.set_mesh_boundary_flags_on_boundary(3, 0, True)
        return {frozenset(st.primitive(d, i).vertex_ids) for d in range(3) for i in range(st.n_primitives(d)) if st.primitive(d, i).on_boundary}
    face = next(i for i in range(st.n_primitives(2)) if st.primitive(2, i).on_boundary)
    ids = frozenset(st.primitive(2, face).vertex_ids)
    st.set_mesh_boundary_flag(2, face, 3)
    flagged = {ids}
    if part == "rim":
        for d in range(2):
            for i in range(st.n_primitives(d)):
                if frozenset(st.primitive(d, i).vertex_ids) <= ids:
                    st.set_mesh_boundary_flag(d, i, 3)
                    flagged.add(frozenset(st.primitive(d, i).vertex_ids))
    return flagged


def selected_truth(st, level, flagged):
    """per local cell, per array entry: the vertices of the lowest-dimensional primitive the point lies on form a flagged set"""
    from oracle import p1_oracle as po

    vid = {tuple(np.round(st.primitive(0, i).coordinates[0], 12)): i for i in range(st.n_primitives(0))}
    n = 1 << level
    ijk = po.cell_coords(level).astype(int)
    out = []
    for c in range(st.n_local_cells):
        ids = [vid[tuple(np.round(p, 12))] for p in st.local_cell(c)[1]]
        sel = np.zeros(len(ijk), dtype=bool)
        for k, (x, y, z) in enumerate(ijk):
            bary = (n - x - y - z, x, y, z)
            sel[k] = frozenset(ids[a] for a in range(4) if bary[a] > 0) in flagged
        out.append(sel)
    return out


def numpy_projection(st, level, before, normal, selected):
    import freesliputil as fu
    import hostutil as hu

    want = [[], [], []]
    for c in range(st.n_local_cells):
        p = hu.cell_points(st.local_cell(c)[1], level)
        nrm = np.zeros((len(p), 3))
        nrm[selected[c]] = np.array([normal(*q) for q in p[selected[c]]], dtype=np.float64).reshape(-1, 3)
        for k, a in enumerate(fu.project_numpy(before[0][c], before[1][c], before[2][c], nrm, selected[c])):
            want[k].append(a)
    return want


CASES = [("tet_1el", l) for l in (0, 1, 2, 3, 4)] + [("cube_6el", 2), ("cube_6el", 3), ("shell60", 2), ("shell60", 3)]


@pytest.mark.parametrize("part", ["face", "rim", "all"])
@pytest.mark.parametrize("normal_kind", ["oblique", "radial"])
@pytest.mark.parametrize("mesh,level", CASES)
def test_project_matches_the_numpy_restatement(env, mesh, level, normal_kind, part):
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    st = make_storage(host, mesh)
    flagged = flag_part_of_the_boundary(st, part)
    normal = oblique if normal_kind == "oblique" else radial_about((0.0, 0.0, 0.0) if mesh == "shell60" else CENTRE)
    proj = host.P1ProjectNormalOperator(st, level, level, normal)
    f = host.P1StokesFunction(st, "f", level, level)
    before = [fu.fill_random(f.components[k], level, 10 * k + level) for k in range(4)]
    selected = selected_truth(st, level, flagged)
    # the library's masks say the same as the geometry
    for a, b in zip(selected, fu.selected_points(st, level, host.FreeslipBoundary)):
        assert np.array_equal(a, b)
    assert sum(int(s.sum()) for s in selected) > 0 or (level == 0 and part == "face") or (level == 1 and part == "face")
    proj.project(f, level, host.FreeslipBoundary)
    got = [hu.download(f.components[k], level) for k in range(4)]
    want = numpy_projection(st, level, before, normal, selected)
    sel_all = np.concatenate(selected)
    for k in range(3):
        g, w = np.concatenate(got[k]), np.concatenate(want[k])
        if sel_all.any():
            err = np.linalg.norm(g[sel_all] - w[sel_all]) / np.linalg.norm(w[sel_all])
            print(f"{mesh} level {level} {normal_kind} {part} component {k}: relative L2 error {err:.3e}")
            assert err <= 1e-13
            assert not np.array_equal(g[sel_all], np.concatenate(before[k])[sel_all]), "nothing was projected"
        # everything that is not selected keeps its bits, the inner points among it
        assert np.array_equal(g[~sel_all], np.concatenate(before[k])[~sel_all])
    assert all(np.array_equal(a, b) for a, b in zip(got[3], before[3])), "the pressure was touched"
    # three P1Functions instead of the composite: the same bits
    f2 = host.P1StokesFunction(st, "f2", level, level)
    for k in range(4):
        hu.upload(f2.components[k], before[k], level)
    proj.project(f2.uvw, level, host.FreeslipBoundary)
    for k in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(hu.download(f2.components[k], level), got[k]))


@pytest.mark.parametrize("mesh,level", [("cube_6el", 3), ("shell60", 2)])
def test_copies_of_shared_boundary_points_stay_identical(env, mesh, level):
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    st = make_storage(host, mesh)
    flag_part_of_the_boundary(st, "all")
    proj = host.P1ProjectNormalOperator(st, level, level, radial_about((0.0, 0.0, 0.0) if mesh == "shell60" else CENTRE))
    f = host.P1StokesFunction(st, "f", level, level)
    for k in range(3):
        fu.fill_random(f.components[k], level, 7 + k)
    proj.project(f, level, host.FreeslipBoundary)
    selected = fu.selected_points(st, level, host.FreeslipBoundary)
    points = [hu.cell_points(st.local_cell(c)[1], level) for c in range(st.n_local_cells)]
    shared = 0
    for k in range(3):
        got = hu.download(f.components[k], level)
        copies = {}
        for c in range(st.n_local_cells):
            for i in np.nonzero(selected[c])[0]:
                copies.setdefault(tuple(np.round(points[c][i], 9)), set()).add(got[c][i].tobytes())
        assert all(len(v) == 1 for v in copies.values()), "the copies of a shared boundary point differ"
        shared += len(copies)
    assert shared > 0


def _interpolated(st, level, fn):
    import hostutil as hu

    return hu.MultiCellOracle(st).interpolate(fn, level)


def test_known_answers_of_the_reference_test_on_the_shell(env):
    """tests/hyteg/freeslip/ProjectNormalTest.cpp, 3-D branch with P1StokesFunction: a radial field vanishes on the free-slip
    boundary (lines 91-94), the tangential field ( -y, x, 0 ) is left alone (line 112)"""
    torch, capi, host = env
    import hostutil as hu

    level = 2
    st = make_storage(host, "shell60")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)

    def interpolant(x, y, z):
        p = np.array([x, y, z])
        r = np.linalg.norm(p)
        return tuple((1.0 if r > 0.75 else -1.0) / r * p)

    proj = host.P1ProjectNormalOperator(st, level, level, interpolant)
    u = host.P1StokesFunction(st, "u", level, level)
    radius = lambda x, y, z: np.sqrt(x * x + y * y + z * z)  # noqa: E731
    for k in range(3):
        comp = lambda x, y, z, k=k: np.where(radius(x, y, z) > 0.75, 1.0, -1.0) / radius(x, y, z) * (x, y, z)[k]  # noqa: E731
        hu.upload(u.components[k], _interpolated(st, level, comp), level)
        u.components[k].sync_shared(level, host.All)
    before = u.dot(u, level, host.FreeslipBoundary)
    proj.project(u, level, host.FreeslipBoundary)
    after = u.dot(u, level, host.FreeslipBoundary)
    print(f"radial field on the free-slip boundary: dot {before:.6e} -> {after:.3e}")
    assert before > 1
    assert after < 1e-14

    tan = host.P1StokesFunction(st, "tan", level, level)
    hu.upload(tan.u, _interpolated(st, level, lambda x, y, z: -y), level)
    hu.upload(tan.v, _interpolated(st, level, lambda x, y, z: x), level)
    tan.u.sync_shared(level, host.All)
    tan.v.sync_shared(level, host.All)
    tan.w.interpolate(0.0, level, host.All)
    u.assign([1.0], [tan], level, host.All)
    assert u.dot(u, level, host.FreeslipBoundary) > 1
    proj.project(u, level, host.FreeslipBoundary)
    diff = host.P1StokesFunction(st, "diff", level, level)
    diff.assign([1.0, -1.0], [u, tan], level, host.All)
    d = diff.dot(diff, level, host.All)
    print(f"tangential field: dot of the difference {d:.3e}")
    assert d < 1e-14


def test_a_selection_that_takes_an_interior_face_raises(env):
    torch, capi, host = env
    import hostutil as hu

    st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
    inner = next(i for i in range(st.n_primitives(2)) if not st.primitive(2, i).on_boundary)
    st.set_mesh_boundary_flag(2, inner, 3)
    proj = host.P1ProjectNormalOperator(st, 2, 2, oblique)
    f = host.P1StokesFunction(st, "f", 2, 2)
    with pytest.raises(host.HytegHostError, match="Cannot project normals if not a boundary face"):
        proj.project(f, 2, host.FreeslipBoundary)


def test_project_with_flag_none_changes_nothing(env):
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    level = 3
    st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)
    proj = host.P1ProjectNormalOperator(st, level, level, oblique)
    f = host.P1StokesFunction(st, "f", level, level)
    before = [fu.fill_random(f.components[k], level, k) for k in range(4)]
    proj.project(f, level, 0)
    for k in range(4):
        assert all(np.array_equal(a, b) for a, b in zip(hu.download(f.components[k], level), before[k]))


def test_project_is_a_timer_of_the_timing_tree(env):
    torch, capi, host = env
    import hostutil as hu

    st = host.Storage.from_gmsh(hu.MESHES / "tet_1el.msh")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)
    proj = host.P1ProjectNormalOperator(st, 2, 2, oblique)
    f = host.P1StokesFunction(st, "f", 2, 2)
    st.enable_timing(True)
    proj.project(f, 2, host.FreeslipBoundary)
    assert '"Project"' in st.timing_json()


def test_an_exception_in_the_normal_function_surfaces(env):
    torch, capi, host = env
    import hostutil as hu

    st = host.Storage.from_gmsh(hu.MESHES / "tet_1el.msh")

    def bad(x, y, z):
        raise ZeroDivisionError("no normal here")

    with pytest.raises(host.HytegHostError, match="normal function failed") as info:
        host.P1ProjectNormalOperator(st, 2, 2, bad)
    assert isinstance(info.value.__cause__, ZeroDivisionError)


def test_a_recorded_project_replays_to_the_same_bits(env):
    """project() allocates, uploads and synchronises nothing, so it can be recorded into a launch graph"""
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    level = 3
    st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)
    proj = host.P1ProjectNormalOperator(st, level, level, radial_about(CENTRE))
    direct, recorded = host.P1StokesFunction(st, "direct", level, level), host.P1StokesFunction(st, "recorded", level, level)
    before = [fu.fill_random(direct.components[k], level, 3 + k) for k in range(3)]
    for k in range(3):
        hu.upload(recorded.components[k], before[k], level)
    proj.project(direct, level, host.FreeslipBoundary)
    want = [hu.download(direct.components[k], level) for k in range(3)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    raw = capi.lib()
    st.set_stream(side.cuda_stream)
    try:
        capi.check(raw.hyteg_hip_graph_begin_capture(side.cuda_stream), "begin_capture")
        try:
            proj.project(recorded, level, host.FreeslipBoundary)
        except BaseException:
            raw.hyteg_hip_graph_abort_capture(side.cuda_stream)
            raise
        graph = ctypes.c_void_p()
        capi.check(raw.hyteg_hip_graph_end_capture(side.cuda_stream, ctypes.byref(graph)), "end_capture")
        assert graph.value, "nothing was recorded"
        # recorded, not run
        for k in range(3):
            assert all(np.array_equal(a, b) for a, b in zip(hu.download(recorded.components[k], level), before[k]))
        capi.check(raw.hyteg_hip_graph_launch(graph, side.cuda_stream), "graph_launch")
        side.synchronize()
        got = [hu.download(recorded.components[k], level) for k in range(3)]
        capi.check(raw.hyteg_hip_graph_destroy(graph), "graph_destroy")
    finally:
        st.set_stream(0)
    for k in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(got[k], want[k]))
        assert not all(np.array_equal(a, b) for a, b in zip(got[k], before[k]))


# ---- P2: the edge-DoF parts (hyteg_hip_p2_edge_project_normal_cells) and P2ProjectNormalOperator ------------------------------------
def consistent_random(points, seed):
    """per cell: random values that depend on the (rounded) coordinates only, so that the copies of a shared DoF agree"""
    rng = np.random.default_rng(seed)
    table = {}
    out = []
    for p in points:
        out.append(np.array([table.setdefault(tuple(q), rng.standard_normal()) for q in np.round(p, 9)]))
    return out


def edge_selected_truth(st, level, flagged):
    """selected_truth for the edge DoFs (array order): the vertices with a non-zero weight at the midpoint form a flagged set"""
    import freesliputil as fu

    vid = {tuple(np.round(st.primitive(0, i).coordinates[0], 12)): i for i in range(st.n_primitives(0))}
    n2 = 2 << level
    m2 = fu.edge_midpoints2(level)
    out = []
    for c in range(st.n_local_cells):
        ids = [vid[tuple(np.round(p, 12))] for p in st.local_cell(c)[1]]
        sel = np.zeros(len(m2), dtype=bool)
        for k, (x, y, z) in enumerate(m2):
            bary = (n2 - x - y - z, x, y, z)
            sel[k] = frozenset(ids[a] for a in range(4) if bary[a] > 0) in flagged
        out.append(sel)
    return out


@pytest.mark.parametrize("part", ["face", "rim", "all"])
@pytest.mark.parametrize("normal_kind", ["oblique", "radial"])
@pytest.mark.parametrize("mesh,level", [("tet_1el", 0), ("tet_1el", 1), ("tet_1el", 2), ("tet_1el", 3), ("tet_1el", 4), ("cube_6el", 2), ("shell60", 2)])
def test_p2_project_matches_the_numpy_restatement(env, mesh, level, normal_kind, part):
    """vertex and edge DoFs of three P2 functions; at level 4 the edge enumeration has 1632 entries (seven workgroups, the last partly
    filled)"""
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    st = make_storage(host, mesh)
    flagged = flag_part_of_the_boundary(st, part)
    normal = oblique if normal_kind == "oblique" else radial_about((0.0, 0.0, 0.0) if mesh == "shell60" else CENTRE)
    proj = host.P2ProjectNormalOperator(st, level, level, normal)
    f = host.TaylorHoodFunction(st, "f", level, level)
    cells = range(st.n_local_cells)
    vpts = [hu.cell_points(st.local_cell(c)[1], level) for c in cells]
    epts = [fu.edge_points(st.local_cell(c)[1], level) for c in cells]
    vsel, esel = selected_truth(st, level, flagged), edge_selected_truth(st, level, flagged)
    for c in cells:  # the library's masks say the same as the geometry
        m = st.mask(c, host.FreeslipBoundary)
        assert np.array_equal(vsel[c], hu.point_mask(level, m & 0x3FFF)) and np.array_equal(esel[c], fu.edge_mask(level, m & 0x3FFF))
    before_v = [consistent_random(vpts, 20 + k) for k in range(3)]
    before_e = [consistent_random(epts, 30 + k) for k in range(3)]
    pressure = consistent_random(vpts, 40)
    for c in cells:
        for k in range(3):
            f.velocity[k].upload(level, before_v[k][c], before_e[k][c], cell=c)
        f.pressure.upload_cell(c, level, pressure[c])
    proj.project(f, level, host.FreeslipBoundary)
    got = [[f.velocity[k].download(level, cell=c) for c in cells] for k in range(3)]

    def normals(points, sel):
        n = np.zeros((len(points), 3))
        n[sel] = np.array([normal(*q) for q in points[sel]], dtype=np.float64).reshape(-1, 3)
        return n

    for part_name, idx, before, pts, sel in (("vertex", 0, before_v, vpts, vsel), ("edge", 1, before_e, epts, esel)):
        want = [[], [], []]
        for c in cells:
            for k, a in enumerate(fu.project_numpy(before[0][c], before[1][c], before[2][c], normals(pts[c], sel[c]), sel[c])):
                want[k].append(a)
        s_all = np.concatenate(sel)
        for k in range(3):
            g, w, b = np.concatenate([got[k][c][idx] for c in cells]), np.concatenate(want[k]), np.concatenate(before[k])
            if s_all.any():
                err = np.linalg.norm(g[s_all] - w[s_all]) / np.linalg.norm(w[s_all])
                print(f"P2 {mesh} level {level} {normal_kind} {part} {part_name} DoFs component {k}: relative L2 error {err:.3e}")
                assert err <= 1e-13
                assert not np.array_equal(g[s_all], b[s_all]), "nothing was projected"
            assert np.array_equal(g[~s_all], b[~s_all])  # bit for bit
    assert sum(int(s.sum()) for s in esel) > 0 or part == "face" and level == 0
    assert all(np.array_equal(f.pressure.download_cell(c, level), pressure[c]) for c in cells), "the pressure was touched"
    # three P2Functions instead of the composite: the same bits, and identical copies of the shared edge DoFs
    u, v, w = (host.P2Function(st, n, level, level) for n in "uvw")
    for c in cells:
        for k, g in enumerate((u, v, w)):
            g.upload(level, before_v[k][c], before_e[k][c], cell=c)
    proj.project([u, v, w], level, host.FreeslipBoundary)
    for k, g in enumerate((u, v, w)):
        copies = {}
        for c in cells:
            a = g.download(level, cell=c)
            assert np.array_equal(a[0], got[k][c][0]) and np.array_equal(a[1], got[k][c][1])
            for i in np.nonzero(esel[c])[0]:
                copies.setdefault(tuple(np.round(epts[c][i], 9)), set()).add(a[1][i].tobytes())
        assert all(len(x) == 1 for x in copies.values()), "the copies of a shared boundary edge DoF differ"


def test_known_answers_of_the_reference_test_for_taylor_hood(env):
    """tests/hyteg/freeslip/ProjectNormalTest.cpp, 3-D branch with P2P1TaylorHoodFunction and P2ProjectNormalOperator"""
    torch, capi, host = env
    import freesliputil as fu
    import hostutil as hu

    level = 2
    st = make_storage(host, "shell60")
    st.set_mesh_boundary_flags_on_boundary(3, 0, True)

    def interpolant(x, y, z):
        p = np.array([x, y, z])
        r = np.linalg.norm(p)
        return tuple((1.0 if r > 0.75 else -1.0) / r * p)

    proj = host.P2ProjectNormalOperator(st, level, level, interpolant)
    cells = range(st.n_local_cells)
    pts = [(np.round(hu.cell_points(st.local_cell(c)[1], level), 12), np.round(fu.edge_points(st.local_cell(c)[1], level), 12)) for c in cells]

    def fill(f, fns):
        for c in cells:
            for k in range(3):
                f.velocity[k].upload(level, fns[k](pts[c][0]), fns[k](pts[c][1]), cell=c)

    def radial(k):
        def fn(p):
            r = np.linalg.norm(p, axis=1)
            return np.where(r > 0.75, 1.0, -1.0) / r * p[:, k]
        return fn

    u = host.TaylorHoodFunction(st, "u", level, level)
    fill(u, [radial(0), radial(1), radial(2)])
    before = u.dot(u, level, host.FreeslipBoundary)
    proj.project(u, level, host.FreeslipBoundary)
    after = u.dot(u, level, host.FreeslipBoundary)
    print(f"Taylor-Hood radial field on the free-slip boundary: dot {before:.6e} -> {after:.3e}")
    assert before > 1
    assert after < 1e-14
    tan = host.TaylorHoodFunction(st, "tan", level, level)
    fill(tan, [lambda p: -p[:, 1], lambda p: p[:, 0], lambda p: 0.0 * p[:, 0]])
    u.assign([1.0], [tan], level, host.All)
    assert u.dot(u, level, host.FreeslipBoundary) > 1
    proj.project(u, level, host.FreeslipBoundary)
    diff = host.TaylorHoodFunction(st, "diff", level, level)
    diff.assign([1.0, -1.0], [u, tan], level, host.All)
    d = diff.dot(diff, level, host.All)
    print(f"Taylor-Hood tangential field: dot of the difference {d:.3e}")
    assert d < 1e-14
