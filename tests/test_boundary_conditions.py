"""Per-primitive boundary conditions without a GPU: BoundaryCondition, mesh boundary flags, the masks they give on the
reference's outflow cube (against a per-point truth computed from coordinates), the exchange classes and their plans, and the
exchange of all classes between ranks."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

from bcutil import CUBE, flags_of, outflow_cube, point_key, point_types, truth
from hostutil import MESHES, cell_points, point_mask
from hyteg_amd import host

ROOT = Path(__file__).resolve().parent.parent
LEVELS = [1, 2, 3]


# ---- 1. BoundaryCondition -------------------------------------------------------------------------------------------
def test_boundary_condition_0123_table_and_default_type():
    bc = host.BoundaryCondition.create_0123()
    assert [bc.boundary_type(f) for f in range(6)] == [host.Inner, host.DirichletBoundary, host.NeumannBoundary,
                                                       host.FreeslipBoundary, host.Inner, host.Inner]
    assert bc.boundary_uid(1).name == "Dirichlet" and bc.boundary_uid(2).name == "Neumann" and bc.boundary_uid(3).name == "Freeslip"
    assert len({bc.boundary_uid(f).id for f in (1, 2, 3, 0)}) == 4
    assert bc.boundary_uid(0) == bc.boundary_uid(17)  # the boundary of the flags that were given none
    empty = host.BoundaryCondition()
    assert [empty.boundary_type(f) for f in (0, 1, 2, 3, 99)] == [host.Inner] * 5


def test_boundary_condition_several_flags_on_one_uid():
    bc = host.BoundaryCondition()
    walls = bc.create_dirichlet("walls", [1, 4, 7])
    out = bc.create_neumann("outflow", 2)
    slip = bc.create_freeslip("lid", [3])
    core = bc.create_inner("core", [9])
    assert [bc.boundary_type(f) for f in (1, 4, 7)] == [host.DirichletBoundary] * 3
    assert [bc.boundary_uid(f) for f in (1, 4, 7)] == [walls] * 3
    assert bc.boundary_type(2) == host.NeumannBoundary and bc.boundary_uid(2) == out
    assert bc.boundary_type(3) == host.FreeslipBoundary and bc.boundary_uid(3) == slip
    assert bc.boundary_type(9) == host.Inner and bc.boundary_uid(9) == core
    assert bc.boundary_type(5) == host.Inner and bc.boundary_uid(5).id == 0
    assert len({walls.id, out.id, slip.id, core.id, 0}) == 5
    with pytest.raises(host.HytegHostError, match="taken"):
        bc.create_neumann("walls", 8)
    with pytest.raises(host.HytegHostError, match="exactly one"):
        bc.create_domain("two", host.Inner | host.NeumannBoundary, [8])


def test_boundary_condition_equality_and_all_inner():
    a, b = host.BoundaryCondition.create_0123(), host.BoundaryCondition.create_0123()
    assert a == b and not (a != b)
    b.create_dirichlet("more", 5)
    assert a != b
    inner = host.BoundaryCondition.create_all_inner()
    assert [inner.boundary_type(f) for f in range(5)] == [host.Inner] * 5
    assert inner == host.BoundaryCondition() and inner != a
    c = host.BoundaryCondition()
    c.create_dirichlet("Dirichlet", 1)
    d = host.BoundaryCondition()
    d.create_neumann("Dirichlet", 1)
    assert c != d  # same flags and names, another type


def test_default_condition_of_the_storage_follows_set_boundary_type():
    st = host.Storage.from_gmsh(CUBE)
    assert st.default_boundary_condition == host.BoundaryCondition.create_0123()
    before = [st.mask(i, host.Inner) for i in range(st.n_local_cells)]
    st.set_boundary_type(host.NeumannBoundary)
    assert st.default_boundary_condition.boundary_type(1) == host.NeumannBoundary
    assert [st.mask(i, host.Inner | host.NeumannBoundary) for i in range(st.n_local_cells)] == [0x7FFF] * st.n_local_cells
    assert [st.mask(i, host.Inner) for i in range(st.n_local_cells)] == before
    st.close()


# ---- the fixture ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube():
    st = outflow_cube("centroid")
    yield st
    st.close()


def test_both_ways_of_flagging_the_outflow_cube_agree(cube):
    one_by_one = outflow_cube("single")
    flags = flags_of(cube)
    assert flags == flags_of(one_by_one)
    one_by_one.close()
    # the face-centre vertex, the four edges from it to the corners and the four faces of z = 1; everything else as by default
    assert [sum(1 for f in fl if f == 2) for fl in flags] == [1, 4, 4]
    default = host.Storage.from_gmsh(CUBE)
    for dim in range(3):
        for i in range(default.n_primitives(dim)):
            p, q = default.primitive(dim, i), cube.primitive(dim, i)
            assert p.flag == (1 if p.on_boundary else 0)
            assert q.flag == (2 if flags[dim][i] == 2 else p.flag) and q.vertex_ids == p.vertex_ids and q.on_boundary == p.on_boundary
            if q.flag == 2:
                assert q.on_boundary and np.all(np.abs(q.coordinates[:, 2] - 1.0) < 1e-12)
    default.close()


def test_location_setters_and_inner_setter():
    st = host.Storage.from_gmsh(CUBE)
    st.set_mesh_boundary_flags_by_vertex_location(5, lambda x, y, z: abs(z) < 1e-12, all_vertices=True)
    st.set_mesh_boundary_flags_by_vertex_location(6, lambda x, y, z: abs(z - 1.0) < 1e-12, all_vertices=False)
    st.set_mesh_boundary_flags_inner(9)
    for dim in range(3):
        for i in range(st.n_primitives(dim)):
            p = st.primitive(dim, i)
            z = p.coordinates[:, 2]
            # flag 6 also went on interior primitives that touch z = 1; the inner setter took them back
            want = 9 if not p.on_boundary else (6 if np.any(np.abs(z - 1.0) < 1e-12) else (5 if np.all(np.abs(z) < 1e-12) else 1))
            assert p.flag == want, (dim, i)
    assert st.boundary_classes == [0, 1, 5, 6, 9]
    with pytest.raises(host.HytegHostError, match="predicate raised") as ei:
        fresh = host.Storage.from_gmsh(CUBE)
        fresh.set_mesh_boundary_flags_by_centroid_location(2, lambda x, y, z: 1 / 0)
    assert isinstance(ei.value.__cause__, ZeroDivisionError)
    st.close()


# ---- 2. masks -------------------------------------------------------------------------------------------------------
FLAGS = [host.Inner, host.DirichletBoundary, host.NeumannBoundary, host.Inner | host.NeumannBoundary, host.All]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("flag", FLAGS)
def test_masks_select_the_points_the_coordinates_select(cube, level, flag):
    want = truth(cube, level, flag)
    for i in range(cube.n_local_cells):
        got = point_mask(level, cube.mask(i, flag))
        assert np.array_equal(got, want[i]), f"cell {i}"


@pytest.mark.parametrize("level", LEVELS)
def test_owned_masks_count_every_selected_point_once(cube, level):
    flag = host.Inner | host.NeumannBoundary
    count = {}
    for i in range(cube.n_local_cells):
        P = cell_points(cube.local_cell(i)[1], level)
        for o in np.nonzero(point_mask(level, cube.mask(i, flag, owned=True)))[0]:
            count[point_key(P[o])] = count.get(point_key(P[o]), 0) + 1
    assert set(count.values()) == {1}
    want = set()
    for i, sel in enumerate(truth(cube, level, flag)):
        want |= {point_key(p) for p in cell_points(cube.local_cell(i)[1], level)[sel]}
    assert set(count) == want and any(abs(k[2] - 1.0) < 1e-12 for k in want)


def test_mask_under_a_condition_of_its_own(cube):
    """the same storage, read by a function whose condition makes the outflow face a wall and the walls free"""
    bc = host.BoundaryCondition()
    bc.create_dirichlet("lid", 2)
    bc.create_neumann("free", 1)
    level = 2
    for i in range(cube.n_local_cells):
        t = point_types(cell_points(cube.local_cell(i)[1], level))
        assert np.array_equal(point_mask(level, cube.mask(i, host.DirichletBoundary, bc=bc)), t == host.NeumannBoundary)
        assert np.array_equal(point_mask(level, cube.mask(i, host.Inner | host.NeumannBoundary, bc=bc)), t != host.NeumannBoundary)
        assert cube.mask(i, host.Inner, bc=host.BoundaryCondition.create_all_inner()) == 0x7FFF
        assert cube.mask(i, host.Boundary, bc=host.BoundaryCondition.create_all_inner()) == 0


# ---- 3. classes and plans -------------------------------------------------------------------------------------------
def _groups(plan):
    gp, eb, eo = plan["group_ptr"], plan["entry_buf"], plan["entry_off"]
    return [tuple((int(eb[e]), int(eo[e])) for e in range(gp[g], gp[g + 1])) for g in range(plan["ngroups"])]


@pytest.mark.parametrize("level", LEVELS)
def test_classes_split_the_boundary_plan_by_flag(cube, level):
    assert cube.boundary_classes == [0, 1, 2]
    assert [host.Storage.plan_key(c, k) for k in (0, 1) for c in (0, 1, 2)] == [0, 1, 4, 2, 3, 6]
    default = host.Storage.from_gmsh(CUBE)
    assert default.boundary_classes == [0, 1]
    for kind in (0, 1):
        key = lambda c: host.Storage.plan_key(c, kind)  # noqa: E731
        assert _groups(cube.plan(level, key(0))) == _groups(default.plan(level, key(0)))
        g1, g2, gd = _groups(cube.plan(level, key(1))), _groups(cube.plan(level, key(2))), _groups(default.plan(level, key(1)))
        assert len(set(g1)) == len(g1) and len(set(g2)) == len(g2) and not set(g1) & set(g2)
        assert sorted(g1 + g2) == sorted(gd)
        # within a class the groups keep the order they had
        assert [g for g in gd if g in set(g1)] == g1 and [g for g in gd if g in set(g2)] == g2
    # every group of class 2 consists of copies of one Neumann point
    pts = [cell_points(cube.local_cell(i)[1], level) for i in range(cube.n_local_cells)]
    g2 = _groups(cube.plan(level, host.Storage.plan_key(2)))
    assert g2
    for g in g2:
        P = np.array([pts[c][o] for c, o in g])
        assert np.all(point_types(P) == host.NeumannBoundary) and np.allclose(P, P[0], atol=1e-13)
    default.close()


@pytest.mark.parametrize("level", LEVELS)
def test_default_plans_do_not_depend_on_setting_the_default_flags(level):
    a, b = host.Storage.from_gmsh(CUBE), host.Storage.from_gmsh(CUBE)
    b.set_mesh_boundary_flags_on_boundary(1, 0)
    assert flags_of(a) == flags_of(b) and a.boundary_classes == b.boundary_classes == [0, 1]
    for key in range(4):
        pa, pb = a.plan(level, key), b.plan(level, key)
        assert pa.keys() == pb.keys()
        for k in pa:
            assert np.array_equal(pa[k], pb[k]), (key, k)
        assert pa["ngroups"] > 0
    for i in range(a.n_local_cells):
        for flag in FLAGS:
            assert a.mask(i, flag) == b.mask(i, flag) and a.mask(i, flag, owned=True) == b.mask(i, flag, owned=True)
    with pytest.raises(host.HytegHostError, match="no such boundary class"):
        a.plan(level, 4)
    a.close()
    b.close()


def test_a_single_tetrahedron_keeps_both_classes():
    st = host.Storage.from_gmsh(MESHES / "tet_1el.msh")
    assert st.boundary_classes == [0, 1]
    assert [st.plan(2, key)["ngroups"] for key in range(4)] == [0, 0, 0, 0]
    st.close()


# ---- 4. send and receive orders between ranks -----------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("level", LEVELS)
def test_send_and_receive_orders_agree_between_ranks_for_every_class(nranks, level):
    sts = [outflow_cube("centroid", r, nranks) for r in range(nranks)]
    assert sum(s.n_local_cells for s in sts) == 24
    pts = [[cell_points(s.local_cell(i)[1], level) for i in range(s.n_local_cells)] for s in sts]
    exchanged = {}
    for cls in range(3):
        assert all(s.boundary_classes == [0, 1, 2] for s in sts)
        plans = [s.plan(level, host.Storage.plan_key(cls)) for s in sts]
        for a in range(nranks):
            pa, off = plans[a], 0
            for k, b in enumerate(pa["peers"]):
                cnt = int(pa["send_count"][k])
                sent = [pts[a][pa["send_buf"][off + j]][pa["send_off"][off + j]] for j in range(cnt)]
                off += cnt
                pb = plans[b]
                assert a in list(pb["peers"]), "peer relation must be symmetric"
                kb = list(pb["peers"]).index(a)
                assert int(pb["recv_count"][kb]) == cnt
                nloc, exp = sts[b].n_local_cells, {}
                gp, eb, eo = pb["group_ptr"], pb["entry_buf"], pb["entry_off"]
                for g in range(pb["ngroups"]):
                    loc = [(eb[e], eo[e]) for e in range(gp[g], gp[g + 1]) if eb[e] < nloc]
                    for e in range(gp[g], gp[g + 1]):
                        if eb[e] == nloc + kb:
                            exp[int(eo[e])] = pts[b][loc[0][0]][loc[0][1]]
                assert sorted(exp) == list(range(cnt))
                for j in range(cnt):
                    assert np.allclose(sent[j], exp[j], atol=1e-13)
                want = {0: host.Inner, 1: host.DirichletBoundary, 2: host.NeumannBoundary}[cls]
                assert cnt == 0 or np.all(point_types(np.array(sent)) == want)
                exchanged[cls] = exchanged.get(cls, 0) + cnt
    assert all(exchanged.get(cls, 0) > 0 for cls in range(3)), exchanged  # every class is really exercised
    for s in sts:
        s.close()


# ---- 5. the exchange of all three classes over gloo -----------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _partials(storage, level):
    out = []
    for i in range(storage.n_local_cells):
        gid, co, _ = storage.local_cell(i)
        P = cell_points(co, level)
        out.append(np.ascontiguousarray((1.0 + gid) * (np.sin(3 * P[:, 0]) + P[:, 1] * 7 - P[:, 2] ** 2)))
    return out


def _reduce(plan, bases, nloc):
    gp, eb, eo = plan["group_ptr"], plan["entry_buf"], plan["entry_off"]
    for g in range(plan["ngroups"]):
        s = 0.0
        for e in range(gp[g], gp[g + 1]):
            s = bases[eb[e]][eo[e]] if e == gp[g] else s + bases[eb[e]][eo[e]]
        for e in range(gp[g], gp[g + 1]):
            if eb[e] < nloc:
                bases[eb[e]][eo[e]] = s


def _worker(rank, world, port, level, q):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    from bcutil import outflow_cube as build
    from hyteg_amd.distributed import DistributedContext

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = build("centroid", rank, world)
        ctx = DistributedContext(st, [level], "cpu")
        assert ctx.class_flags == [0, 1, 2] and ctx.n_classes == 3
        arrays, nloc, moved = _partials(st, level), st.n_local_cells, []
        for cls in range(3):
            key = st.plan_key(cls)
            p = ctx.plans[(level, key)]
            segs = []
            if len(p["peers"]):
                send = ctx.send_tensor(level, key)
                packed = np.array([arrays[b][o] for b, o in zip(p["send_buf"], p["send_off"])])
                send[: len(packed)] = torch.from_numpy(packed)
                ctx.exchange(level, key)
                recv, off = ctx.recv_tensor(level, key).numpy(), 0
                for k in range(len(p["peers"])):
                    segs.append(recv[off: off + int(p["recv_count"][k])])
                    off += int(p["recv_count"][k])
            moved.append(int(p["total_send"]))
            _reduce(p, arrays + segs, nloc)
        q.put((rank, [st.local_cell(i)[0] for i in range(nloc)], arrays, moved))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_exchange_of_all_classes_over_gloo_reproduces_the_single_process_sums():
    import torch.multiprocessing as mp

    level, world = 2, 2
    st = outflow_cube("centroid")
    ref = _partials(st, level)
    for cls in range(3):
        _reduce(st.plan(level, st.plan_key(cls)), ref, st.n_local_cells)
    st.close()
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, level, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p_ in procs:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    seen = 0
    for rank, gids, arrays, moved in results:
        assert all(m > 0 for m in moved), f"rank {rank} sent nothing for some class: {moved}"
        for gid, arr in zip(gids, arrays):
            assert np.array_equal(arr, ref[gid]), f"rank {rank} cell {gid}"  # bit for bit: fixed summation order
            seen += 1
    assert seen == 24


# ---- 6. the flags are fixed once something depends on them ----------------------------------------------------------
def test_flag_setters_throw_once_a_plan_exists():
    st = host.Storage.from_gmsh(CUBE)
    st.set_mesh_boundary_flag(2, 0, 7)  # fine: nothing depends on the flags yet
    st.mask(0, host.All)  # a mask is computed, not cached
    st.set_mesh_boundary_flag(2, 0, st.primitive(2, 0).flag)
    st.plan(2, 0)
    for call in (lambda: st.set_mesh_boundary_flag(0, 0, 3),
                 lambda: st.set_mesh_boundary_flags_on_boundary(1, 0),
                 lambda: st.set_mesh_boundary_flags_inner(0),
                 lambda: st.set_mesh_boundary_flags_by_vertex_location(2, lambda x, y, z: True),
                 lambda: st.set_mesh_boundary_flags_by_centroid_location(2, lambda x, y, z: True)):
        with pytest.raises(host.HytegHostError, match="flags are fixed"):
            call()
    st.close()
    st = host.Storage.from_gmsh(CUBE)
    with pytest.raises(host.HytegHostError, match="dimension"):
        st.set_mesh_boundary_flag(3, 0, 1)
    with pytest.raises(host.HytegHostError):
        st.set_mesh_boundary_flag(0, st.n_vertices, 1)
    st.close()
