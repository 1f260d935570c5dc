"""GPU tests of the function reductions of the host layer through Python: P1Function / P2Function .sum, .max_value, .min_value,
.max_magnitude and .reduce against numpy on the downloaded cell arrays.

Mask rule (the reference's, VertexDoFFunction.cpp:1841-1847 and :1914-1918): the sums count every DoF once -- the owned masks
st.mask(i, flag, owned=True), cell interiors only if the flag contains Inner -- while max, min and max magnitude always include
the cell interiors and take the macro-faces, -edges and -vertices from the owned mask for the flag.
Sums: |got - fsum| <= 1e-12 * sum|x| (the project's fp64 parity bound; the summation order differs from fsum's by a small
multiple of eps * sum|x|).  Extrema: exactly numpy's."""
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MESHES = ROOT / "hyteg_amd" / "data" / "meshes"
DBL_MAX = float(np.finfo(np.float64).max)
INNER_BIT = 1 << 14


def _host():
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch

    from hyteg_amd import host

    assert torch.cuda.is_available()
    return host


def _selections(level, p2):
    """per part of the function (vertex DoFs; edge DoFs of a P2 function): the point class of every array entry"""
    from oracle import p1_oracle as po

    return [po.slot_of_points(level)] + ([po.edge_classes(level)] if p2 else [])


def _make(host, st, level, p2):
    """a function with seeded standard normals, a different field per GLOBAL cell (so every rank layout sees the same data);
    returns (function, {global cell id: [vertex array, edge array]})"""
    f = (host.P2Function if p2 else host.P1Function)(st, "f", level, level)
    data = {}
    for c in range(st.n_local_cells):
        gid = st.local_cell(c)[0]
        rng = np.random.default_rng(500 + gid)
        parts = [rng.standard_normal(len(s)) for s in _selections(level, p2)]
        data[gid] = parts
        if p2:
            f.upload(level, parts[0], parts[1], cell=c)
        else:
            f.upload_cell(c, level, parts[0])
    return f, data


def _expected(st_single, data, level, p2, flag):
    """numpy on the arrays of ALL cells with the masks of the single-rank storage: (sum, sum_abs, min, max, magnitude)"""
    summed, extreme = [], []
    for c in range(st_single.n_local_cells):
        gid = st_single.local_cell(c)[0]
        owned = st_single.mask(c, flag, owned=True)
        for cls, arr in zip(_selections(level, p2), data[gid]):
            summed.append(arr[((owned >> cls) & 1).astype(bool)])
            extreme.append(arr[(((owned | INNER_BIT) >> cls) & 1).astype(bool)])
    s, e = np.concatenate(summed), np.concatenate(extreme)
    return (math.fsum(s), math.fsum(np.abs(s)), e.min() if e.size else DBL_MAX, e.max() if e.size else -DBL_MAX,
            np.abs(e).max() if e.size else 0.0)


def _check(got, want, tag):
    print(tag, "sum err", abs(got[0] - want[0]), "sum_abs err", abs(got[1] - want[1]), "bound", 1e-12 * want[1])
    assert abs(got[0] - want[0]) <= 1e-12 * want[1], tag
    assert abs(got[1] - want[1]) <= 1e-12 * want[1], tag
    assert tuple(got[2:]) == tuple(want[2:]), tag


@pytest.mark.parametrize("p2", [False, True], ids=["P1", "P2"])
@pytest.mark.parametrize("level", [2, 4])
@pytest.mark.parametrize("mesh", ["regular_octahedron_8el", "cube_6el"])
def test_reductions_match_numpy_for_every_flag(mesh, level, p2):
    host = _host()
    st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
    f, data = _make(host, st, level, p2)
    for flag in (host.All, host.Inner, host.DirichletBoundary, host.Inner | host.DirichletBoundary):
        want = _expected(st, data, level, p2, flag)
        r = f.reduce(level, flag)
        _check(tuple(r), want, (mesh, level, p2, flag))
        # the five methods are views of the same pass
        assert f.sum(level, flag) == r.sum and f.sum(level, flag, absolute=True) == r.sum_abs
        assert (f.min_value(level, flag), f.max_value(level, flag), f.max_magnitude(level, flag)) == (r.min, r.max, r.max_magnitude)
        assert tuple(f.reduce(level, flag, mpi_reduce=False)) == tuple(r)  # one rank
        if flag == host.DirichletBoundary:
            # no interior in the sums, every interior in the extrema
            assert all(not (st.mask(c, flag, owned=True) & INNER_BIT) for c in range(st.n_local_cells))
    for c in range(st.n_local_cells):  # nothing was written
        got = f.download(level, cell=c) if p2 else [f.download_cell(c, level)]
        assert all(np.array_equal(g, w) for g, w in zip(got, data[st.local_cell(c)[0]]))
    f.close()
    st.close()


@pytest.mark.parametrize("p2", [False, True], ids=["P1", "P2"])
def test_spikes_follow_the_references_flag_rule(p2):
    """a spike inside a macro-cell is returned with flag = DirichletBoundary (the reference does not flag-test macro-cells for
    the extrema) but is not part of that flag's sum; a spike on a boundary vertex is not returned with flag = Inner"""
    from oracle import p1_oracle as po

    host = _host()
    level = 2
    st = host.Storage.from_gmsh(MESHES / "regular_octahedron_8el.msh")
    f = (host.P2Function if p2 else host.P1Function)(st, "f", level, level)
    nv, ne = po.cell_size(level), po.edge_array_size(level)
    cell = 3
    inner = int(np.flatnonzero(po.slot_of_points(level) == 14)[0])
    v, e = np.zeros(nv), np.zeros(ne)
    v[inner] = -1000.0
    f.upload(level, v, e, cell=cell) if p2 else f.upload_cell(cell, level, v)
    for flag in (host.DirichletBoundary, host.Inner, host.All):
        assert f.min_value(level, flag) == -1000.0 and f.max_magnitude(level, flag) == 1000.0 and f.max_value(level, flag) == 0.0
    assert f.sum(level, host.DirichletBoundary) == 0.0 and f.sum(level, host.Inner) == -1000.0
    # a boundary vertex of cell 0 (the lowest-numbered cell owns its primitives)
    slot = next(s for s in range(10, 14) if st.mask(0, host.DirichletBoundary, owned=True) >> s & 1)
    N = po.width(level)
    corner = [(0, 0, 0), (N - 1, 0, 0), (0, N - 1, 0), (0, 0, N - 1)][slot - 10]
    v = np.zeros(nv)
    v[po.cell_index(level, *corner)] = 5000.0
    f.upload(level, np.zeros(nv), e, cell=cell) if p2 else f.upload_cell(cell, level, np.zeros(nv))
    f.upload(level, v, e, cell=0) if p2 else f.upload_cell(0, level, v)
    assert f.max_value(level, host.Inner) == 0.0 and f.max_magnitude(level, host.Inner) == 0.0 and f.sum(level, host.Inner) == 0.0
    for flag in (host.DirichletBoundary, host.All):
        assert f.max_value(level, flag) == 5000.0 and f.sum(level, flag) == 5000.0
    if p2:
        # an edge DoF inside the cell: same rule for the edge-DoF part
        e2 = np.zeros(ne)
        e2[int(np.flatnonzero(po.edge_classes(level) == 14)[-1])] = 7000.0
        f.upload(level, np.zeros(nv), e2, cell=cell)
        # (the vertex spike of 5000 is still there: it is all that the boundary's sum sees)
        assert f.max_value(level, host.DirichletBoundary) == 7000.0 and f.sum(level, host.DirichletBoundary) == 5000.0
        assert f.sum(level, host.Inner) == 7000.0 and f.sum(level, host.All) == 12000.0
    f.close()
    st.close()


@pytest.mark.parametrize("p2", [False, True], ids=["P1", "P2"])
@pytest.mark.parametrize("mesh,level", [("regular_octahedron_8el", 2), ("cube_6el", 3), ("tet_1el", 4)])
def test_sum_of_ones_counts_the_dofs(mesh, level, p2):
    host = _host()
    st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
    one = (host.P2Function if p2 else host.P1Function)(st, "one", level, level)
    one.interpolate(1.0, level, host.All)
    n = st.number_of_dofs(level, p2=p2)
    assert n == st.number_of_dofs(level, p2=p2, global_=False) and n > 0
    assert one.sum(level) == float(n) == one.dot(one, level) == one.sum(level, host.All, absolute=True)
    assert tuple(one.reduce(level)[2:]) == (1.0, 1.0, 1.0)
    one.close()
    st.close()


# ---- two ranks sharing the one GPU over gloo ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


FLAGS_2RANKS = (15, 2)  # All, DirichletBoundary


def _worker(rank, world, port, level, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    from hyteg_amd import host
    from hyteg_amd.distributed import DistributedContext

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = host.Storage.from_gmsh(MESHES / "regular_octahedron_8el.msh", rank, world)
        st.set_stream(torch.cuda.current_stream().cuda_stream)
        DistributedContext(st, [level], torch.device("cuda", 0), transport="hooks")
        out = {}
        for p2 in (False, True):
            f, _ = _make(host, st, level, p2)
            for flag in FLAGS_2RANKS:
                g, loc = f.reduce(level, flag), f.reduce(level, flag, mpi_reduce=False)
                assert (f.sum(level, flag), f.sum(level, flag, absolute=True)) == (g.sum, g.sum_abs)
                assert (f.min_value(level, flag), f.max_value(level, flag), f.max_magnitude(level, flag)) == (g.min, g.max, g.max_magnitude)
                assert (f.min_value(level, flag, mpi_reduce=False), f.max_value(level, flag, mpi_reduce=False),
                        f.max_magnitude(level, flag, mpi_reduce=False)) == (loc.min, loc.max, loc.max_magnitude)
                out[(p2, flag)] = (tuple(g), tuple(loc))
            f.close()
        q.put((rank, out))
        dist.barrier()
    except BaseException as e:  # the parent fails at once instead of waiting for the queue
        q.put(("error", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_reduce_to_the_single_rank_values():
    import torch.multiprocessing as mp

    host = _host()
    level, world = 2, 2
    st = host.Storage.from_gmsh(MESHES / "regular_octahedron_8el.msh")
    ref = {}
    for p2 in (False, True):
        f, data = _make(host, st, level, p2)
        for flag in FLAGS_2RANKS:
            ref[(p2, flag)] = tuple(f.reduce(level, flag))
            _check(ref[(p2, flag)], _expected(st, data, level, p2, flag), ("single rank", p2, flag))
        f.close()
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, level, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    for _ in range(world):
        results.append(q.get(timeout=240))
        assert results[-1][0] != "error", results[-1]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    by_rank = dict(results)
    for key, want in ref.items():
        locals_ = [by_rank[r][key][1] for r in range(world)]
        for r in range(world):
            g = by_rank[r][key][0]
            assert g[2:] == want[2:], (key, r)  # exact
            assert abs(g[0] - want[0]) <= 1e-12 * want[1] and abs(g[1] - want[1]) <= 1e-12 * want[1], (key, r)
        # mpi_reduce=False: the rank-local values, which differ between the ranks and combine to the global ones
        assert locals_[0][2:] != locals_[1][2:] and locals_[0][:2] != locals_[1][:2], key
        assert (min(l[2] for l in locals_), max(l[3] for l in locals_), max(l[4] for l in locals_)) == want[2:], key
        assert abs(sum(l[0] for l in locals_) - want[0]) <= 1e-12 * want[1], key
    st.close()
