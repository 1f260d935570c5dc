"""GPU tests of the preconditioned CGSolver and the symmetric smoothers through the host layer (hyteg_amd/host/solvers.hpp, host.py):
against plain CG, against the numpy restatement of the loop (tests/pcgutil.py) with the reference's forward + backward sweep
schedule (hostutil.GlobalSweepOracle), against the existing smooth_sor entry points, with multigrid as preconditioner for P1 and P2,
and on two ranks."""
import functools
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MESHES = ROOT / "hyteg_amd" / "data" / "meshes"
TOL = 1e-10


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    host.lib()
    return torch, host, po, hu


@functools.lru_cache(maxsize=None)
def _glob(mesh, level):
    import hostutil as hu

    v, c = hu.read_msh(MESHES / f"{mesh}.msh")
    return hu.GlobalSweepOracle(v, c, level)


class _P1Problem:
    """A x = b on one level: random right-hand side (default_rng(1)), random Dirichlet values, zero start inside"""

    def __init__(self, host, hu, mesh, level, min_level=None):
        import pcgutil

        self.host, self.hu, self.level = host, hu, level
        self.glob = _glob(mesh, level)
        self.free = pcgutil.free_points(self.glob)
        rng = np.random.default_rng(1)
        self.b_g = rng.standard_normal(self.glob.ndof)
        self.x0_g = np.where(self.free, 0.0, rng.standard_normal(self.glob.ndof))
        lo = level if min_level is None else min_level
        self.st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
        self.A = host.P1ConstantOperator(self.st, lo, level)
        self.x, self.b, self.r = (host.P1Function(self.st, n, lo, level) for n in ("x", "b", "r"))
        hu.upload(self.b, self.glob.to_cells(self.b_g), level)

    def start(self):
        self.hu.upload(self.x, self.glob.to_cells(self.x0_g), self.level)

    def solution(self):
        """the global vector; all copies of a shared point hold the same bits, the Dirichlet values are those of the start"""
        got = self.hu.download(self.x, self.level)
        g = self.glob.to_global(got)
        for idx, a in zip(self.glob.gidx, got):
            assert np.array_equal(a, g[idx])
        assert np.array_equal(g[~self.free], self.x0_g[~self.free])
        return g

    def residual_norm(self):
        host, L = self.host, self.level
        self.r.interpolate(0.0, L)
        self.A.apply(self.x, self.r, L, host.Inner)
        self.r.assign([1.0, -1.0], [self.b, self.r], L, host.Inner)
        return float(np.sqrt(self.r.dot(self.r, L, host.Inner)))

    def solve(self, solver):
        """from the start value; returns (global solution, iterations, initial and final true residual norm)"""
        self.start()
        res0 = self.residual_norm()
        solver.solve(self.A, self.x, self.b, self.level)
        return self.solution(), solver.iterations, res0, self.residual_norm()

    def close(self, *solvers):
        for o in (*solvers, self.x, self.b, self.r, self.A, self.st):
            o.close()


def test_identity_preconditioner_reproduces_plain_cg(env):
    torch, host, po, hu = env
    pr = _P1Problem(host, hu, "cube_6el", 3)
    L = pr.level
    plain = host.Solver.cg(pr.st, L, L, 3, 1e-14)
    identity = host.Solver.smoother(pr.st, L, L, host.IDENTITY)
    pcg = host.Solver.cg(pr.st, L, L, 3, 1e-14, preconditioner=identity)
    want, its_plain, _, _ = pr.solve(plain)
    got, its, _, _ = pr.solve(pcg)
    assert its_plain == 3 and its == 3
    assert np.abs(want - pr.x0_g).max() > 1e-3 * np.abs(want).max()  # three iterations moved x
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the three composed calls instead of the fused update: the same iterates
    pcg.set_use_fused_update(False)
    composed, its, _, _ = pr.solve(pcg)
    assert its == 3 and np.abs(composed - want).max() <= 1e-12 * np.abs(want).max()
    pr.close(plain, pcg, identity)


@pytest.mark.parametrize("mesh,level", [("cube_6el", 2), ("tet_1el", 3)])
def test_symmetric_gauss_seidel_preconditioner_matches_the_restated_loop(env, mesh, level):
    torch, host, po, hu = env
    import pcgutil

    pr = _P1Problem(host, hu, mesh, level)
    glob = pr.glob
    want, its, iterates = pcgutil.pcg(glob.matvec, pcgutil.sweep_preconditioner(glob), pr.x0_g, pr.b_g, pr.free, 3)
    assert its == 3
    sgs = host.Solver.smoother(pr.st, level, level, host.SYMMETRIC_GAUSS_SEIDEL)
    pcg = host.Solver.cg(pr.st, level, level, 3, 1e-14, preconditioner=sgs)
    got, its_gpu, _, _ = pr.solve(pcg)
    assert its_gpu == 3
    assert np.abs(want - pr.x0_g).max() > 1e-3 * np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    pr.close(pcg, sgs)


@pytest.mark.parametrize("mesh,level", [("cube_6el", 2), ("tet_1el", 3)])
def test_symmetric_gauss_seidel_preconditioner_saves_iterations(env, mesh, level):
    """the CPU restatement takes 10 against 18 (cube_6el, level 2) and 9 against 19 (tet_1el, level 3) iterations"""
    torch, host, po, hu = env
    pr = _P1Problem(host, hu, mesh, level)
    plain = host.Solver.cg(pr.st, level, level, 200, TOL)
    sgs = host.Solver.smoother(pr.st, level, level, host.SYMMETRIC_GAUSS_SEIDEL)
    pcg = host.Solver.cg(pr.st, level, level, 200, TOL, preconditioner=sgs)
    _, its_plain, res0, res_plain = pr.solve(plain)
    _, its_pcg, res0_pcg, res_pcg = pr.solve(pcg)
    print(f"{mesh} level {level}: plain {its_plain}, symmetric Gauss-Seidel {its_pcg} iterations; residuals {res0:.3e} -> {res_plain:.3e}, {res_pcg:.3e}")
    assert res0 == res0_pcg and res0 > 1.0  # the relative tolerance decides, not the absolute one
    assert 0 < its_pcg < its_plain < 200
    assert res_plain <= 10 * TOL * res0 and res_pcg <= 10 * TOL * res0
    pr.close(plain, pcg, sgs)


def test_symmetric_sor_smoother_is_a_forward_and_a_backward_sweep(env):
    torch, host, po, hu = env
    mesh, level, relax = "cube_6el", 3, 1.3
    pr = _P1Problem(host, hu, mesh, level)
    glob = pr.glob
    u_g = np.random.default_rng(2).standard_normal(glob.ndof)
    y = host.P1Function(pr.st, "y", level, level)
    hu.upload(pr.x, glob.to_cells(u_g), level)
    hu.upload(y, glob.to_cells(u_g), level)
    ssor = host.Solver.smoother(pr.st, level, level, host.SYMMETRIC_SOR, relax)
    ssor.solve(pr.A, pr.x, pr.b, level)
    pr.A.smooth_sor(y, pr.b, relax, level, host.Inner | host.NeumannBoundary, False)
    pr.A.smooth_sor(y, pr.b, relax, level, host.Inner | host.NeumannBoundary, True)
    got, two_calls = hu.download(pr.x, level), hu.download(y, level)
    for a, w in zip(got, two_calls):
        assert np.array_equal(a, w)
    want = glob.sweep(glob.sweep(u_g, pr.b_g, relax, False), pr.b_g, relax, True)
    assert np.abs(want - u_g).max() > 1e-3 * np.abs(want).max()
    for g, a in zip(glob.gidx, got):
        assert np.abs(a - want[g]).max() <= 1e-12 * np.abs(want).max()
    # symmetric Gauss-Seidel is the same with relax = 1, whatever relax is passed
    sgs = host.Solver.smoother(pr.st, level, level, host.SYMMETRIC_GAUSS_SEIDEL, 0.7)
    hu.upload(pr.x, glob.to_cells(u_g), level)
    sgs.solve(pr.A, pr.x, pr.b, level)
    want = glob.sweep(glob.sweep(u_g, pr.b_g, 1.0, False), pr.b_g, 1.0, True)
    for g, a in zip(glob.gidx, hu.download(pr.x, level)):
        assert np.abs(a - want[g]).max() <= 1e-12 * np.abs(want).max()
    y.close()
    pr.close(ssor, sgs)


def _upload_p2(po, hu, st, f, level, fn):
    for c in range(st.n_local_cells):
        gid, co, nnc = st.local_cell(c)
        f.upload(level, fn(hu.cell_points(co, level)), fn(po.edge_midpoints(co, level)), c)


def _rough(p):
    return np.sin(37.0 * p[:, 0] + 11.0 * p[:, 1]) * np.cos(23.0 * p[:, 2]) + p[:, 0] * p[:, 1]


def test_p2_symmetric_sor_smoother_is_the_two_smooth_sor_calls(env):
    torch, host, po, hu = env
    level, relax = 2, 1.3
    st = host.Storage.from_gmsh(MESHES / "cube_6el.msh")
    A = host.P2ElementwiseLaplaceOperator(st, level, level)
    A.compute_inverse_diagonal()
    x, y, b = (host.P2Function(st, n, level, level) for n in ("x", "y", "b"))
    _upload_p2(po, hu, st, x, level, _rough)
    _upload_p2(po, hu, st, y, level, _rough)
    _upload_p2(po, hu, st, b, level, lambda p: np.cos(5.0 * p[:, 0] + p[:, 1]) - p[:, 2])
    before = [x.download(level, c) for c in range(st.n_local_cells)]
    ssor = host.P2Solver.smoother(st, level, level, host.SYMMETRIC_SOR, relax)
    ssor.solve(A, x, b, level)
    A.smooth_sor(y, b, relax, level, host.Inner | host.NeumannBoundary, False)
    A.smooth_sor(y, b, relax, level, host.Inner | host.NeumannBoundary, True)
    changed = False
    for c in range(st.n_local_cells):
        (gv, ge), (wv, we) = x.download(level, c), y.download(level, c)
        assert np.array_equal(gv, wv) and np.array_equal(ge, we)
        changed = changed or not np.array_equal(gv, before[c][0])
    assert changed
    for o in (ssor, x, y, b, A, st):
        o.close()


def test_symmetric_gauss_seidel_is_a_symmetric_operator_on_one_macro_cell(env):
    """B u = the smoother applied to a zero start with right-hand side u, tet_1el level 3: <Bu,v> = <u,Bv>"""
    torch, host, po, hu = env
    pr = _P1Problem(host, hu, "tet_1el", 3)
    L, glob, free = pr.level, pr.glob, pr.free
    rng = np.random.default_rng(3)
    sgs = host.Solver.smoother(pr.st, L, L, host.SYMMETRIC_GAUSS_SEIDEL)

    def B(w):
        hu.upload(pr.b, glob.to_cells(w), L)
        pr.x.interpolate(0.0, L)
        sgs.solve(pr.A, pr.x, pr.b, L)
        return glob.to_global(hu.download(pr.x, L))

    u, v = (np.where(free, rng.standard_normal(glob.ndof), 0.0) for _ in range(2))
    Bu, Bv = B(u), B(v)
    assert np.linalg.norm(Bu) > 0 and not Bu[~free].any()
    assert abs(float(Bu @ v) - float(u @ Bv)) <= 1e-12 * np.linalg.norm(Bu) * np.linalg.norm(v)
    pr.close(sgs)


def test_p1_multigrid_preconditioner_saves_iterations(env):
    """regular_octahedron_8el, levels 0-3: CG preconditioned by one V(1,1) cycle with symmetric Gauss-Seidel against plain CG"""
    torch, host, po, hu = env
    pr = _P1Problem(host, hu, "regular_octahedron_8el", 3, min_level=0)
    plain = host.Solver.cg(pr.st, 0, 3, 200, TOL)
    gmg = host.Solver.gmg(pr.st, 0, 3, smoother=host.SYMMETRIC_GAUSS_SEIDEL, pre=1, post=1)
    pcg = host.Solver.cg(pr.st, 0, 3, 200, TOL, preconditioner=gmg)
    _, its_plain, res0, res_plain = pr.solve(plain)
    _, its_pcg, _, res_pcg = pr.solve(pcg)
    print(f"P1 regular_octahedron_8el levels 0-3: plain CG {its_plain}, V(1,1) preconditioned CG {its_pcg} iterations")
    assert 0 < its_pcg < its_plain < 200
    assert res_plain <= 10 * TOL * res0 and res_pcg <= 10 * TOL * res0
    pr.close(plain, pcg, gmg)


def test_p2_multigrid_preconditioner_saves_iterations(env):
    """cube_6el, P2 levels 2-3: the same statement with P2Solver"""
    torch, host, po, hu = env
    lo, L = 2, 3
    st = host.Storage.from_gmsh(MESHES / "cube_6el.msh")
    A = host.P2ElementwiseLaplaceOperator(st, lo, L)
    A.compute_inverse_diagonal()
    x, b, r = (host.P2Function(st, n, lo, L) for n in ("x", "b", "r"))
    _upload_p2(po, hu, st, b, L, _rough)

    def residual():
        r.interpolate(0.0, L)
        A.apply(x, r, L, host.Inner)
        r.assign([1.0, -1.0], [b, r], L, host.Inner)
        return float(np.sqrt(r.dot(r, L, host.Inner)))

    x.interpolate(0.0, L)
    res0 = residual()
    its_plain = A.cg_solve(x, b, L, 400, TOL)
    res_plain = residual()
    gmg = host.P2Solver(st, lo, L, pre=1, post=1, smoother=host.SYMMETRIC_GAUSS_SEIDEL)
    pcg = host.P2Solver.cg(st, lo, L, 400, TOL, preconditioner=gmg)
    x.interpolate(0.0, L)
    pcg.solve(A, x, b, L)
    its_pcg, res_pcg = pcg.iterations, residual()
    print(f"P2 cube_6el levels 2-3: plain CG {its_plain}, V(1,1) preconditioned CG {its_pcg} iterations; residual {res0:.3e} -> {res_plain:.3e}, {res_pcg:.3e}")
    assert res0 > 1e-2
    assert 0 < its_pcg < its_plain < 400
    assert res_plain <= 10 * TOL * res0 and res_pcg <= 10 * TOL * res0
    # without a preconditioner P2Solver.cg is the plain solver
    same = host.P2Solver.cg(st, lo, L, 400, TOL)
    x.interpolate(0.0, L)
    same.solve(A, x, b, L)
    assert same.iterations == its_plain
    for o in (same, pcg, gmg, x, b, r, A, st):
        o.close()


# ---- two ranks on the one GPU (the set-up of test_gpu_distributed.py) ------------------------------------------------------------
RANK_MESH, RANK_LEVEL = "cube_6el", 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranked(host, st, level):
    """three iterations of CG preconditioned with symmetric Gauss-Seidel; returns {global cell id: x}, iterations"""
    sys.path.insert(0, str(ROOT / "tests"))
    from hostutil import cell_points

    A = host.P1ConstantOperator(st, level, level)
    x, b = host.P1Function(st, "x", level, level), host.P1Function(st, "b", level, level)
    for c in range(st.n_local_cells):
        gid, co, nnc = st.local_cell(c)
        P = cell_points(co, level)
        b.upload_cell(c, level, np.ascontiguousarray(np.sin(5 * P[:, 0] + 2 * P[:, 1]) + P[:, 2] * P[:, 0]))
        x.upload_cell(c, level, np.ascontiguousarray(np.cos(3 * P[:, 0] - P[:, 1]) * (1.0 + P[:, 2])))
    b.sync_shared(level, host.All)
    x.sync_shared(level, host.All)
    x.interpolate(0.0, level, host.Inner)  # zero inside, the function's values on the Dirichlet boundary
    sgs = host.Solver.smoother(st, level, level, host.SYMMETRIC_GAUSS_SEIDEL)
    pcg = host.Solver.cg(st, level, level, 3, 1e-14, preconditioner=sgs)
    pcg.solve(A, x, b, level)
    return {st.local_cell(c)[0]: x.download_cell(c, level) for c in range(st.n_local_cells)}, pcg.iterations


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist

    from hyteg_amd import host
    from hyteg_amd.distributed import DistributedContext

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = host.Storage.from_gmsh(MESHES / f"{RANK_MESH}.msh", rank, world)
        st.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx = DistributedContext(st, [2, 3], torch.device("cuda", 0))  # noqa: F841
        out = _run_ranked(host, st, RANK_LEVEL)
        st.check_transport()
        q.put((rank,) + out)
        dist.barrier()
    except BaseException as e:  # the parent fails at once instead of waiting for the queue
        q.put(("error", rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_reproduce_the_one_rank_iterates(env):
    """every copy of a shared point is updated, on whichever rank it lives, and counted once in <r,r>"""
    torch, host, po, hu = env
    import torch.multiprocessing as mp

    st = host.Storage.from_gmsh(MESHES / f"{RANK_MESH}.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    ref, its = _run_ranked(host, st, RANK_LEVEL)
    assert its == 3
    scale = max(np.abs(a).max() for a in ref.values())
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    for _ in range(world):
        results.append(q.get(timeout=240))
        assert results[-1][0] != "error", results[-1]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cells = 0
    for rank, xs, rank_its in results:
        assert rank_its == 3
        for gid, arr in xs.items():
            assert np.abs(arr - ref[gid]).max() <= 1e-12 * scale, (rank, gid)
            cells += 1
    assert cells == st.n_cells
