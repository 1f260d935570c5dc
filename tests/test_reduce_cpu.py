"""CPU-only tests of the function reductions (sum, min, max, max magnitude): the C-ABI declares and exports the entries and
rejects bad arguments before any GPU work, PrimitiveStorage::allreduceMax is exact over gloo and runs in rounds of at most 16
slots on the transport's sum, and the DoF counts equal the closed forms."""
import math
import os
import re
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
MESHES = ROOT / "hyteg_amd" / "data" / "meshes"
DBL_MAX = float(np.finfo(np.float64).max)
# per rank: values with negatives and -DBL_MAX; column 1 is negative on every rank, column 2 is -DBL_MAX on every rank
VALUES = np.array([[1.5, -3.0, -DBL_MAX, -DBL_MAX, 0.0, 7.25],
                   [-2.0, -1.0, -DBL_MAX, 4.0, -0.5, 7.25],
                   [0.25, -8.0, -DBL_MAX, -1e-300, -DBL_MAX, DBL_MAX]])


def test_header_declares_and_library_exports_the_reduce_entries():
    import ctypes

    from hyteg_amd import capi, host

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for sym in ("hyteg_hip_reduce_workspace_bytes", "hyteg_hip_p1_reduce_cells", "hyteg_hip_p2_edge_reduce_cells"):
        assert re.search(rf"\b{sym}\s*\(", text), sym
        assert hasattr(raw, sym) and sym in capi.SIGNATURES
    for k, name in enumerate(("SUM", "SUM_ABS", "MIN", "MAX", "MAX_ABS", "COUNT")):
        assert re.search(rf"#define HYTEG_HIP_REDUCE_{name} {k}\b", text), name
    assert capi.reduce_workspace_bytes() >= capi.HYTEG_HIP_MAX_BATCH * capi.REDUCE_COUNT * 8
    htext = (ROOT / "include" / "hyteg_host.h").read_text()
    hraw = ctypes.CDLL(str(host._LIB_PATH))
    for sym in ("hyteg_host_p1_reduce", "hyteg_host_p2_reduce", "hyteg_host_storage_allreduce_max",
                "hyteg_host_storage_p1_number_of_dofs", "hyteg_host_storage_p2_number_of_dofs"):
        assert re.search(rf"\b{sym}\s*\(", htext) and hasattr(hraw, sym), sym


@pytest.mark.parametrize("form", ["vertex", "edge"])
def test_bad_arguments_are_rejected_before_any_gpu_work(form):
    """EINVAL on the host (this machine may have no GPU: anything that reached the device would fail differently)"""
    from hyteg_amd import capi

    fn = capi.p1_reduce_cells if form == "vertex" else capi.p2_edge_reduce_cells
    a, m, r, w = [4096], [0x7FFF], 8192, 16384
    for args in ((None, 3, m, r, w), (a, 3, None, r, w), (a, 3, m, None, w), (a, 3, m, r, None), ([0], 3, m, r, w)):
        with pytest.raises(capi.HytegHipError, match=r"code -?\d+\): .*null"):
            fn(*args)
    for n in (0, capi.HYTEG_HIP_MAX_BATCH + 1):
        with pytest.raises(capi.HytegHipError, match="ncells"):
            fn([4096] * n, 3, [0x7FFF] * n, r, w)
    for level in (-1, 12 if form == "vertex" else 10):
        with pytest.raises(capi.HytegHipError, match="level out of range"):
            fn(a, level, m, r, w)
    if form == "edge":
        assert capi.p2_edge_array_size(9) > 0 and capi.p2_edge_array_size(10) == 0  # HYTEG_HIP_P2_MAX_LEVEL is 9


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from hyteg_amd import host
    from hyteg_amd.distributed import DistributedContext

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = host.Storage.from_gmsh(MESHES / "regular_octahedron_8el.msh", rank, world)
        DistributedContext(st, [2], "cpu")
        mx = st.allreduce_max(VALUES[rank])
        mn = -st.allreduce_max(-VALUES[rank])
        q.put((rank, list(mx), list(mn)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_max_over_gloo_is_the_numpy_maximum(world):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_max, want_min = VALUES[:world].max(axis=0), VALUES[:world].min(axis=0)
    assert want_max[1] < 0 and want_max[2] == -DBL_MAX
    for rank, mx, mn in results:
        assert mx == list(want_max), rank  # exact: x + 0 == x
        assert mn == list(want_min), rank


def _recording_hooks(st):
    calls = []
    st.set_hooks(lambda level, key: None, lambda level, key: None, lambda values, n: calls.append(n))
    return calls


def test_one_rank_returns_the_value_without_a_transport_call():
    from hyteg_amd import host

    st = host.Storage.from_gmsh(MESHES / "tet_1el.msh")
    assert list(st.allreduce_max([-5.0, -DBL_MAX])) == [-5.0, -DBL_MAX]  # no transport set at all
    calls = _recording_hooks(st)
    assert list(st.allreduce_max([-5.0, 2.0])) == [-5.0, 2.0] and calls == []
    st.close()


@pytest.mark.parametrize("world,rank", [(17, 0), (20, 17), (24, 15), (24, 16), (24, 23)])
def test_allreduce_max_runs_in_rounds_of_at_most_16_slots(world, rank):
    """a rank of a world of more than 16 whose all-reduce hook leaves the vector as it is (every other rank contributes 0):
    ceil(world / 16) calls of at most 16 values, and the rank's own value comes back out of its slot"""
    from hyteg_amd import host

    st = host.Storage.from_gmsh(MESHES / "cube_24el.msh", rank, world)
    calls = _recording_hooks(st)
    assert list(st.allreduce_max([3.5])) == [3.5]
    assert calls == [min(16, world - f) for f in range(0, world, 16)]
    assert len(calls) == math.ceil(world / 16) and max(calls) <= 16
    # against the zeros that stand for the other ranks a negative value loses
    del calls[:]
    assert list(st.allreduce_max([-2.0])) == [0.0] and len(calls) == math.ceil(world / 16)
    st.close()


def _binom(n, k):
    return math.comb(n, k) if n >= k else 0


@pytest.mark.parametrize("mesh", ["tet_1el", "cube_6el", "regular_octahedron_8el"])
def test_dof_counts_equal_the_closed_forms(mesh):
    from hyteg_amd import host

    st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
    nv, ne, nf, nc = st.n_vertices, st.n_edges, st.n_faces, st.n_cells
    for level in range(0, 4):
        n = 1 << level
        p1 = nv + ne * (n - 1) + nf * _binom(n - 1, 2) + nc * _binom(n - 1, 3)
        # edge DoFs: n per macro-edge, 3 n (n - 1) / 2 inside a macro-face, the rest of the cell's 6 tet(n) + tet(n - 1) inside it
        tet = lambda w: w * (w + 1) * (w + 2) // 6
        edge = ne * n + nf * (3 * n * (n - 1) // 2) + nc * (6 * tet(n) + tet(n - 1) - 6 * n - 4 * (3 * n * (n - 1) // 2))
        for global_ in (True, False):  # one rank: local == global
            assert st.number_of_dofs(level, global_=global_) == p1, (level, global_)
            assert st.number_of_dofs(level, p2=True, global_=global_) == p1 + edge, (level, global_)
    st.close()
    # several ranks: the local counts add up to the global count
    for world in (2, 3):
        parts = []
        for rank in range(world):
            s = host.Storage.from_gmsh(MESHES / f"{mesh}.msh", rank, world)
            parts.append((s.number_of_dofs(2, global_=False), s.number_of_dofs(2, p2=True, global_=False)))
            total = (s.number_of_dofs(2), s.number_of_dofs(2, p2=True))
            s.close()
        assert tuple(map(sum, zip(*parts))) == total
