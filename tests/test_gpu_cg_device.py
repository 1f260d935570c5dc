"""GPU tests of the conjugate gradient pieces that live on the device (hyteg_amd/csrc/p1_batch.hip), entry by entry:
the scalar recurrences (hyteg_hip_cg_scalars), the dot product that runs them in its own launch, the vector updates that read
their coefficients from device memory, and the one-launch solve -- against a Python restatement of the header comment, the
host-scalar kernels, and a numpy CG on a matrix built from the CPU oracle alone."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASKS = [0x7FFF, 0x4000 | 0x2A5, 0x3FFF]
FACES = 0x03C0  # the four macro-face slots


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host, po


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- hyteg_hip_cg_scalars -------------------------------------------------------------------------------------------------
PRSOLD, PAP, RR, ALPHA, NEG_ALPHA, BETA, RES_START, DONE, ITERATIONS, ONE = range(10)


def _cg_scalars_ref(s, phase, rel_tol, abs_tol):
    """include/hyteg_hip.h, the comment above enum hyteg_hip_cg_slot, restated.  Phase 0 is also where an iteration starts:
    it resets ITERATIONS, ALPHA, NEG_ALPHA and BETA and sets ONE (the coefficient the update p = 1 r + beta p reads)."""
    s = list(s)
    done = s[DONE] != 0.0
    if phase == 0:
        s[PRSOLD] = s[RR]
        s[RES_START] = math.sqrt(s[RR])
        s[DONE] = 1.0 if s[RES_START] < abs_tol else 0.0
        s[ITERATIONS], s[ONE] = 0.0, 1.0
        s[ALPHA] = s[NEG_ALPHA] = s[BETA] = 0.0
    elif phase == 1:
        alpha = 0.0 if done else s[PRSOLD] / s[PAP]
        s[ALPHA], s[NEG_ALPHA] = alpha, -alpha
    elif not done:
        s[ITERATIONS] += 1.0
        sq = math.sqrt(s[RR])
        if sq / s[RES_START] < rel_tol or sq < abs_tol:
            s[DONE] = 1.0
        else:
            s[BETA] = s[RR] / s[PRSOLD]
            s[PRSOLD] = s[RR]
    return s


def _slots(**named):
    """sixteen slots with distinct, recognisable values; the named ones overridden"""
    s = [0.5 + 0.125 * k for k in range(16)]
    s[DONE] = 0.0
    for k, v in named.items():
        s[globals()[k]] = v
    return s


def _assert_slots(got, want):
    for k in range(16):
        if k == RES_START:
            assert abs(got[k] - want[k]) <= 2 * np.spacing(abs(want[k])), (k, got[k], want[k])
        else:
            assert got[k] == want[k] and math.copysign(1.0, got[k]) == math.copysign(1.0, want[k]), (k, got[k], want[k])


# every threshold comparison below is at least 1 % away from its tolerance
CG_SCALAR_CASES = {
    "phase 0, residual above abs_tol": (0, _slots(RR=7.3, DONE=1.0), 1e-8, 1e-3, dict(DONE=0.0)),
    "phase 0, residual below abs_tol": (0, _slots(RR=2.5e-9), 1e-8, 1e-3, dict(DONE=1.0)),
    "phase 1, running": (1, _slots(PRSOLD=3.7, PAP=11.1), 1e-8, 1e-3, dict(ALPHA=3.7 / 11.1, NEG_ALPHA=-(3.7 / 11.1))),
    "phase 1, done": (1, _slots(PRSOLD=3.7, PAP=11.1, DONE=1.0), 1e-8, 1e-3, dict(ALPHA=0.0, NEG_ALPHA=-0.0)),
    "phase 2, continuing": (2, _slots(RR=0.9, PRSOLD=1.7, RES_START=3.0, ITERATIONS=4.0), 1e-8, 1e-3,
                            dict(BETA=0.9 / 1.7, PRSOLD=0.9, ITERATIONS=5.0, DONE=0.0)),
    "phase 2, stops by rel_tol": (2, _slots(RR=1e-6, PRSOLD=1.7, RES_START=3.0, ITERATIONS=4.0), 1e-3, 1e-9,
                                  dict(DONE=1.0, ITERATIONS=5.0, BETA=_slots()[BETA], PRSOLD=1.7)),
    "phase 2, stops by abs_tol": (2, _slots(RR=1e-6, PRSOLD=1.7, RES_START=3.0, ITERATIONS=4.0), 1e-9, 2e-3,
                                  dict(DONE=1.0, ITERATIONS=5.0, BETA=_slots()[BETA], PRSOLD=1.7)),
    "phase 2, already done": (2, _slots(RR=0.9, PRSOLD=1.7, RES_START=3.0, ITERATIONS=4.0, DONE=1.0), 1e-8, 1e-3,
                              dict(DONE=1.0, ITERATIONS=4.0, BETA=_slots()[BETA], PRSOLD=1.7)),
}


@pytest.mark.parametrize("case", list(CG_SCALAR_CASES))
def test_cg_scalars_phases_follow_the_header(env, case):
    torch, capi, host, po = env
    phase, before, rel_tol, abs_tol, expect = CG_SCALAR_CASES[case]
    want = _cg_scalars_ref(before, phase, rel_tol, abs_tol)
    for k, v in expect.items():  # the restatement does what the case is named for
        assert want[globals()[k]] == v, k
    if phase == 2 and before[DONE] == 0.0:  # distance of the two convergence tests from their thresholds
        sq = math.sqrt(before[RR])
        assert abs(sq / before[RES_START] / rel_tol - 1.0) >= 0.01 and abs(sq / abs_tol - 1.0) >= 0.01
    if phase == 0:
        assert abs(math.sqrt(before[RR]) / abs_tol - 1.0) >= 0.01
    s = _dev(torch, np.array(before))
    capi.cg_scalars(s.data_ptr(), phase, rel_tol, abs_tol)
    _assert_slots(s.cpu().numpy().tolist(), want)
    if case == "phase 2, already done":
        assert s.cpu().numpy().tolist() == before


def test_cg_scalars_rejects_bad_arguments(env):
    torch, capi, host, po = env
    s = _dev(torch, np.zeros(16))
    for phase in (-1, 3):
        with pytest.raises(capi.HytegHipError):
            capi.cg_scalars(s.data_ptr(), phase, 0.0, 0.0)
    with pytest.raises(capi.HytegHipError):
        capi.cg_scalars(None, 0, 0.0, 0.0)
    assert (capi.HYTEG_HIP_CG_PRSOLD, capi.HYTEG_HIP_CG_PAP, capi.HYTEG_HIP_CG_RR, capi.HYTEG_HIP_CG_ALPHA, capi.HYTEG_HIP_CG_NEG_ALPHA,
            capi.HYTEG_HIP_CG_BETA, capi.HYTEG_HIP_CG_RES_START, capi.HYTEG_HIP_CG_DONE, capi.HYTEG_HIP_CG_ITERATIONS, capi.HYTEG_HIP_CG_ONE,
            capi.HYTEG_HIP_CG_SLOTS) == (PRSOLD, PAP, RR, ALPHA, NEG_ALPHA, BETA, RES_START, DONE, ITERATIONS, ONE, 16)


# ---- hyteg_hip_p1_dot_cells_cg ----------------------------------------------------------------------------------------------
def _full_tiles_per_cell(level, capacity=256):
    N = (1 << level) + 1
    return sum(((N - z) * (N - z + 1) // 2 + capacity - 1) // capacity for z in range(N))


@pytest.mark.parametrize("level,where", [(2, "batch_dot_kernel"), (5, "batch_dot_final_kernel")])
@pytest.mark.parametrize("slot", ["PAP", "RR"])
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_dot_cells_cg_is_the_dot_product_followed_by_the_recurrence(env, level, where, slot, phase):
    """up to 64 workgroups the recurrence runs in the workgroup of batch_dot_kernel that finishes last, above in batch_dot_final_kernel"""
    torch, capi, host, po = env
    ncells, slot = 3, globals()[slot]
    assert (ncells * _full_tiles_per_cell(level) <= 64) == (where == "batch_dot_kernel")
    n = po.cell_size(level)
    rng = np.random.default_rng(level)
    ta, tb = _dev(torch, rng.standard_normal((ncells, n))), _dev(torch, rng.standard_normal((ncells, n)))
    if slot == RR:
        tb = ta  # <r, r>: positive, as the square root of phases 0 and 2 needs
    pa, pb = [ta[c].data_ptr() for c in range(ncells)], [tb[c].data_ptr() for c in range(ncells)]
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    res = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
    capi.p1_dot_cells(pa, pb, level, MASKS, res.data_ptr(), ws.data_ptr())
    dot = float(res.cpu()[0])
    assert dot != 0.0 and dot != 1e300 and (slot == PAP or dot > 0.0)
    rel_tol, abs_tol = 1e-8, 1e-3
    before = _slots(PRSOLD=1.7 * abs(dot), RES_START=3.0 * math.sqrt(abs(dot)), ITERATIONS=4.0)
    before[slot] = 1e300  # the launch has to overwrite it
    s = _dev(torch, np.array(before))
    capi.p1_dot_cells_cg(pa, pb, level, MASKS, s.data_ptr(), slot, phase, rel_tol, abs_tol, ws.data_ptr())
    got = s.cpu().numpy().tolist()
    assert got[slot] == dot  # the bits of p1_dot_cells
    after_dot = list(before)
    after_dot[slot] = dot
    _assert_slots(got, _cg_scalars_ref(after_dot, phase, rel_tol, abs_tol))


def test_dot_cells_cg_rejects_other_slots(env):
    torch, capi, host, po = env
    a = _dev(torch, np.ones(po.cell_size(2)))
    s = _dev(torch, np.array(_slots()))
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    for slot in (PRSOLD, ALPHA, NEG_ALPHA, BETA, RES_START, DONE, ITERATIONS, ONE, -1, 16):
        with pytest.raises(capi.HytegHipError):
            capi.p1_dot_cells_cg([a.data_ptr()], [a.data_ptr()], 2, [0x7FFF], s.data_ptr(), slot, 1, 0.0, 0.0, ws.data_ptr())
    with pytest.raises(capi.HytegHipError):
        capi.p1_dot_cells_cg([a.data_ptr()], [a.data_ptr()], 2, [0x7FFF], s.data_ptr(), PAP, 3, 0.0, 0.0, ws.data_ptr())
    assert s.cpu().numpy().tolist() == _slots()


# ---- hyteg_hip_p1_vector_cells_dev ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2, 4])
@pytest.mark.parametrize("op", [0, 1])
def test_vector_cells_dev_has_the_bits_of_the_host_scalar_call(env, level, op):
    torch, capi, host, po = env
    n = po.cell_size(level)
    rng = np.random.default_rng(20 + level)
    src, d0 = _dev(torch, rng.standard_normal((4, 3, n))), _dev(torch, rng.standard_normal((3, n)))
    values = _slots(NEG_ALPHA=-0.3125, ONE=1.0, BETA=0.7, ALPHA=0.3125)
    s = _dev(torch, np.array(values))
    slots = [NEG_ALPHA, ONE, BETA, ALPHA]
    for nsrc in (1, 2, 3, 4):
        ptrs = [[src[k, c].data_ptr() for c in range(3)] for k in range(nsrc)]
        a, b = d0.clone(), d0.clone()
        capi.p1_vector_cells_dev(op, [a[c].data_ptr() for c in range(3)], ptrs, [s.data_ptr() + 8 * k for k in slots[:nsrc]], level, MASKS)
        capi.p1_vector_cells(op, [b[c].data_ptr() for c in range(3)], ptrs, [values[k] for k in slots[:nsrc]], level, MASKS)
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(ah, bh)
        assert not np.array_equal(ah, d0.cpu().numpy())
    assert s.cpu().numpy().tolist() == values


def test_vector_cells_dev_rejects_other_ops_and_null_pointers(env):
    torch, capi, host, po = env
    a, b = _dev(torch, np.zeros(po.cell_size(2))), _dev(torch, np.ones(po.cell_size(2)))
    s = _dev(torch, np.ones(16))
    for op in (2, 3):
        with pytest.raises(capi.HytegHipError):
            capi.p1_vector_cells_dev(op, [a.data_ptr()], [[b.data_ptr()]], [s.data_ptr()], 2, [0x7FFF])
    with pytest.raises(capi.HytegHipError):
        capi.p1_vector_cells_dev(0, [a.data_ptr()], [[b.data_ptr()], [b.data_ptr()]], [s.data_ptr(), None], 2, [0x7FFF])
    with pytest.raises(capi.HytegHipError):
        capi.p1_vector_cells_dev(0, [a.data_ptr()], [[b.data_ptr()]], None, 2, [0x7FFF])
    assert not a.cpu().numpy().any()


# ---- hyteg_hip_p1_cg_small_cells --------------------------------------------------------------------------------------------
LEVEL = 3  # 165 entries per cell, 35 of them inner points


@functools.lru_cache(maxsize=None)
def _cell_operators():
    """per cell of regular_octahedron_8el: (stencil table [15][15], matrix [165][165]) with the matrix built column by column
    from the oracle's apply on unit vectors: the inner stencil on inner rows, the cell's own slot stencils on shell rows"""
    import hostutil as hu
    from oracle import p1_oracle as po

    v, c = hu.read_msh(hu.MESHES / "regular_octahedron_8el.msh")
    n = po.cell_size(LEVEL)
    out = []
    for cv in c:
        co = v[cv].reshape(12)
        slots, inner = po.assemble_cell_slot_stencils(co, LEVEL).reshape(14, 15), po.assemble_cell_stencil(co, LEVEL)
        M = np.zeros((n, n))
        for j in range(n):
            e, col = np.zeros(n), np.zeros(n)
            e[j] = 1.0
            po.apply_cell(col, e, LEVEL, inner, po.REPLACE)
            po.apply_cell_boundary(col, e, LEVEL, slots.reshape(-1), po.MASK_SHELL, po.REPLACE)
            M[:, j] = col
        out.append((np.vstack([slots, inner[None, :]]), M))
    return out


def _numpy_cg(A, b, x0, max_iter, rel_tol, abs_tol):
    """CGSolver::solve (CGSolver.hpp:91-140) with the identity preconditioner; returns x, iterations, the recurrence residual
    norm at exit, the initial residual norm, and residual / initial residual after every iteration"""
    x = x0.copy()
    r = b - A @ x
    p = r.copy()
    prsold = float(r @ r)
    res_start = res = math.sqrt(prsold)
    its, ratios = 0, []
    if res_start < abs_tol:
        return x, its, res, res_start, ratios
    for i in range(max_iter):
        ap = A @ p
        alpha = prsold / float(p @ ap)
        x += alpha * p
        r -= alpha * ap
        rsnew = float(r @ r)
        res, its = math.sqrt(rsnew), i + 1
        ratios.append(res / res_start)
        if res / res_start < rel_tol or res < abs_tol:
            break
        p = r + (rsnew / prsold) * p
        prsold = rsnew
    return x, its, res, res_start, ratios


class _Problem:
    """`ncells` independent cells (no shared points): random x (unselected entries are Dirichlet data entering through A x),
    random b; the reference system is block diagonal over the selected entries, right-hand side b - A_SD x_D"""

    def __init__(self, masks, seed):
        import hostutil as hu

        ops = _cell_operators()
        rng = np.random.default_rng(seed)
        self.masks, self.n = list(masks), ops[0][1].shape[0]
        nc = len(self.masks)
        self.tabs = np.array([ops[c % len(ops)][0] for c in range(nc)])
        self.M = [ops[c % len(ops)][1] for c in range(nc)]
        self.sel = [hu.point_mask(LEVEL, m) for m in self.masks]
        self.x0 = [rng.standard_normal(self.n) for _ in range(nc)]
        self.b = [rng.standard_normal(self.n) for _ in range(nc)]
        sizes = [int(s.sum()) for s in self.sel]
        self.off = np.concatenate([[0], np.cumsum(sizes)])
        self.A = np.zeros((self.off[-1], self.off[-1]))
        self.rhs = np.zeros(self.off[-1])
        for c in range(nc):
            S, lo, hi = self.sel[c], self.off[c], self.off[c + 1]
            self.A[lo:hi, lo:hi] = self.M[c][np.ix_(S, S)]
            self.rhs[lo:hi] = self.b[c][S] - self.M[c][np.ix_(S, ~S)] @ self.x0[c][~S]
        assert np.abs(self.A - self.A.T).max() <= 1e-14 * np.abs(self.A).max() and np.linalg.eigvalsh(self.A).min() > 0  # SPD
        self.xs0 = np.concatenate([self.x0[c][self.sel[c]] for c in range(nc)])

    def reference(self, max_iter, rel_tol, abs_tol):
        return _numpy_cg(self.A, self.rhs, self.xs0, max_iter, rel_tol, abs_tol)

    def solve_on_gpu(self, torch, capi, max_iter, rel_tol, abs_tol):
        nc = len(self.masks)
        x, b, tab = _dev(torch, np.array(self.x0)), _dev(torch, np.array(self.b)), _dev(torch, self.tabs.reshape(-1))
        info = torch.full((2,), 1e300, dtype=torch.float64, device="cuda")
        capi.p1_cg_small_cells([x[c].data_ptr() for c in range(nc)], [b[c].data_ptr() for c in range(nc)], LEVEL, tab.data_ptr(), self.masks,
                               self.masks, max_iter, rel_tol, abs_tol, info.data_ptr())
        xh = x.cpu().numpy()
        for c in range(nc):  # Dirichlet data and everything else the mask does not select: bit-identical to the input
            assert np.array_equal(xh[c][~self.sel[c]], self.x0[c][~self.sel[c]])
        return np.concatenate([xh[c][self.sel[c]] for c in range(nc)]), info.cpu().numpy()

    def true_residual(self, xs):
        return float(np.linalg.norm(self.rhs - self.A @ xs))


REL_TOL = 1e-13
# (masks, seed); the seeds are the ones of 1..40 whose numpy CG has its residual ratio furthest from REL_TOL both at the exit and one
# iteration before it: factors 2.7 / 4.7 (24 iterations), 1.6 / 1.6 (59) and 1.3 / 1.5 (82); the test asserts at least 1 %
CG_SMALL_CASES = {
    "inner points, Dirichlet shell": ([1 << 14], 10),
    "inner and face points": ([0x4000 | FACES], 28),
    "13 cells, LDS above 48 KiB": ([1 << 14, 0x4000 | FACES, 0x4000 | 0x0140] * 4 + [1 << 14], 13),
}


@pytest.mark.parametrize("case", list(CG_SMALL_CASES))
def test_cg_small_three_iterations_match_the_numpy_cg(env, case):
    torch, capi, host, po = env
    masks, seed = CG_SMALL_CASES[case]
    pr = _Problem(masks, seed)
    assert len(masks) * pr.n <= capi.p1_cg_small_max_entries()
    assert (3 * len(masks) * pr.n * 8 > 48 * 1024) == (len(masks) == 13)
    assert all((~s).any() and np.abs(x[~s]).min() > 0 for s, x in zip(pr.sel, pr.x0))  # non-zero Dirichlet data
    want, its, res, res_start, ratios = pr.reference(3, 0.0, 0.0)
    got, info = pr.solve_on_gpu(torch, capi, 3, 0.0, 0.0)
    assert its == 3 and info[0] == 3.0
    assert abs(info[1] - res) <= 1e-12 * res
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    for c in range(len(masks)):  # each cell against its own part of the reference
        lo, hi = pr.off[c], pr.off[c + 1]
        assert hi > lo and np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(want - pr.xs0).max() > 1e-3 * np.abs(want).max()  # three iterations moved x


@pytest.mark.parametrize("case", list(CG_SMALL_CASES))
def test_cg_small_converges_to_the_relative_tolerance(env, case):
    """The true residual b - A x of the kernel's x, computed on the CPU with the reference matrix, against
    REL_TOL * |b - A x0| times a margin for the drift between the recurrence residual and the true one: ten times the drift
    of the numpy CG at its exit, (true residual) / (recurrence residual), measured in the test.  Measured on the CPU: 0.997
    (inner points), 0.998 (inner and face points), 0.999 (13 cells) -- no drift at these sizes, so the margin is 10."""
    torch, capi, host, po = env
    masks, seed = CG_SMALL_CASES[case]
    pr = _Problem(masks, seed)
    want, its, res, res_start, ratios = pr.reference(300, REL_TOL, 0.0)
    assert 3 < its < 300 and ratios[-1] < REL_TOL <= ratios[-2]
    assert abs(ratios[-1] / REL_TOL - 1.0) >= 0.01 and abs(ratios[-2] / REL_TOL - 1.0) >= 0.01
    drift = pr.true_residual(want) / res
    got, info = pr.solve_on_gpu(torch, capi, 300, REL_TOL, 0.0)
    print(f"{case}: numpy its {its} ratios {ratios[-2]:.3e} {ratios[-1]:.3e} drift {drift:.3f}; gpu its {info[0]} res {info[1]:.3e} "
          f"true {pr.true_residual(got):.3e} bound {REL_TOL * res_start * 10.0 * max(1.0, drift):.3e}")
    assert info[0] == float(its)
    assert info[1] / res_start < REL_TOL
    assert pr.true_residual(got) <= REL_TOL * res_start * 10.0 * max(1.0, drift)
    exact = np.linalg.solve(pr.A, pr.rhs)
    # x - x* = A^-1 (A x - rhs): bounded by the residual bound over the smallest eigenvalue
    assert np.linalg.norm(got - exact) <= REL_TOL * res_start * 10.0 * max(1.0, drift) / np.linalg.eigvalsh(pr.A).min() + 1e-13 * np.linalg.norm(exact)


def test_cg_small_already_converged(env):
    """b = 0, x = 0 and the host layer's default abs_tol: no iteration, no division by <p, A p> = 0"""
    torch, capi, host, po = env
    n = po.cell_size(LEVEL)
    tab = _dev(torch, _cell_operators()[0][0].reshape(-1))
    x, b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    info = torch.full((2,), 1e300, dtype=torch.float64, device="cuda")
    capi.p1_cg_small_cells([x.data_ptr()], [b.data_ptr()], LEVEL, tab.data_ptr(), [1 << 14], [1 << 14], 300, REL_TOL, 1e-16, info.data_ptr())
    xh = x.cpu().numpy()
    assert np.isfinite(xh).all() and not xh.any()
    assert info.cpu().numpy().tolist() == [0.0, 0.0]


def test_cg_small_rejects_problems_that_do_not_fit(env):
    torch, capi, host, po = env
    n = po.cell_size(LEVEL)
    ncells = capi.p1_cg_small_max_entries() // n + 1
    assert ncells <= capi.HYTEG_HIP_MAX_BATCH and ncells * n > capi.p1_cg_small_max_entries() == 4096
    x, b = torch.zeros((ncells, n), dtype=torch.float64, device="cuda"), torch.ones((ncells, n), dtype=torch.float64, device="cuda")
    tab = _dev(torch, np.array([_cell_operators()[0][0]] * ncells).reshape(-1))
    with pytest.raises(capi.HytegHipError):
        capi.p1_cg_small_cells([x[c].data_ptr() for c in range(ncells)], [b[c].data_ptr() for c in range(ncells)], LEVEL, tab.data_ptr(),
                               [1 << 14] * ncells, [1 << 14] * ncells, 10, 0.0, 0.0)
    assert not x.cpu().numpy().any()


# ---- the one-launch solve through the host layer, non-zero Dirichlet data ---------------------------------------------------------
@pytest.mark.parametrize("mesh,level", [("regular_octahedron_8el", 2), ("cube_24el", 3)])
def test_single_launch_cg_with_dirichlet_data_solves_the_global_system(env, mesh, level):
    """CGSolver with single_launch on a problem whose boundary values are not zero: the boundary enters through A x only.
    cube_24el at level 3 is 3960 of the 4096 entries the kernel holds (95 KiB of LDS) with both exchange classes in use.
    Checked against hostutil.GlobalSweepOracle's matrix: residual criterion of the direct tests, the dense solution, and
    bit-identical copies of every shared point."""
    torch, capi, host, po = env
    import hostutil as hu

    v, c = hu.read_msh(hu.MESHES / f"{mesh}.msh")
    glob = hu.GlobalSweepOracle(v, c, level)
    K = np.zeros((glob.ndof, glob.ndof))
    for i, row in enumerate(glob.rows):
        for j, w in row.items():
            K[i, j] = w
    bnd = np.array(glob.boundary)
    assert bnd.any() and (~bnd).any()
    st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
    assert st.n_local_cells * po.cell_size(level) <= capi.p1_cg_small_max_entries()
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    A = host.P1ConstantOperator(st, level, level)
    x, b, xe = (host.P1Function(st, n, level, level) for n in ("x", "b", "xe"))
    xe_h = []
    for k in range(st.n_local_cells):
        gid, co, nnc = st.local_cell(k)
        P = hu.cell_points(co, level)
        xe_h.append(np.ascontiguousarray(np.sin(3 * P[:, 0]) * P[:, 1] + P[:, 2] ** 2 + 0.5))
    xe_g = glob.to_global(xe_h)
    xe_h = glob.to_cells(xe_g)  # the copies of a shared point carry the same bits
    assert np.abs(xe_g[bnd]).min() > 0
    hu.upload(xe, xe_h, level)
    A.apply(xe, b, level, host.Inner)
    x.assign([1.0], [xe], level, host.DirichletBoundary)  # x: zero inside, the Dirichlet values on the boundary
    x0 = glob.to_global(hu.download(x, level))
    assert np.array_equal(x0[bnd], xe_g[bnd]) and not x0[~bnd].any()
    b_g = glob.to_global(hu.download(b, level))
    Kii, rhs = K[np.ix_(~bnd, ~bnd)], b_g[~bnd] - K[np.ix_(~bnd, bnd)] @ x0[bnd]
    want, its, res, res_start, ratios = _numpy_cg(Kii, rhs, x0[~bnd], 300, REL_TOL, 0.0)
    assert 3 < its < 300
    drift = float(np.linalg.norm(rhs - Kii @ want)) / res
    cg = host.Solver.cg(st, level, level, 300, REL_TOL)
    cg.set_use_device_scalars(True, single_launch=True)
    cg.solve(A, x, b, level)
    got = hu.download(x, level)
    got_g = glob.to_global(got)
    for g, a in zip(glob.gidx, got):
        assert np.array_equal(a, got_g[g])  # all copies of a shared point: the same bits
    assert np.array_equal(got_g[bnd], xe_g[bnd])  # Dirichlet values untouched
    true_res = float(np.linalg.norm(rhs - Kii @ got_g[~bnd]))
    bound = REL_TOL * res_start * 10.0 * max(1.0, drift)
    print(f"{mesh}: numpy its {its} drift {drift:.3f}; gpu its {cg.iterations} true residual {true_res:.3e} bound {bound:.3e}")
    assert true_res <= bound
    exact = np.linalg.solve(Kii, rhs)
    assert np.linalg.norm(got_g[~bnd] - exact) <= bound / np.linalg.eigvalsh(Kii).min() + 1e-13 * np.linalg.norm(exact)
    assert np.abs(exact - xe_g[~bnd]).max() <= 1e-9 * np.abs(xe_g).max()  # and that is the function b was made from
    for o in (cg, x, b, xe, A, st):
        o.close()
