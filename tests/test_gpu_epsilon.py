"""GPU tests of the epsilon-operator kernels (include/hyteg_hip.h section b-5) through the C-ABI on one non-axis-aligned macro-cell,
entry by entry against the numpy element loop of tests/epsilonutil.py (pinned by tests/test_epsilon_restatement.py).
Inputs: u, v, w in [-1, 1], mu in [0.5, 50].  Criteria per component: relative L2 <= 1e-12 and max entry error <= 1e-12 * max|dst|
(the project's fp64 parity bar); entries outside the class mask are bit-identical to the sentinel the destination was filled with."""
import functools

import numpy as np
import pytest

import epsilonutil as eu
from conftest import SKEW_TET

pytestmark = pytest.mark.gpu
TOL = 1e-12
TET = SKEW_TET  # all six micro-cell types differ
MASKS = {"all": eu.MASK_ALL, "inner": eu.MASK_INNER, "shell": eu.MASK_SHELL, "face1": 1 << 7, "edge4": 1 << 4}
OMEGA = 2.0 / 3.0


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi


def dev3(torch, a):
    """three device arrays (copies: the shared cases are read-only) and their pointers"""
    t = [torch.from_numpy(np.array(x, dtype=np.float64)).to("cuda") for x in a]
    return t, [x.data_ptr() for x in t]


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")


def host3(t):
    return np.stack([x.cpu().numpy() for x in t])


def sentinel(n):
    return np.stack([7.0 + 3.0 * np.sin(0.37 * np.arange(n) + c) for c in range(3)])


@functools.lru_cache(maxsize=None)
def case(level):
    """src (3, n) in [-1, 1], mu in [0.5, 50] and the restatement's ( A src ) on all points: computed once per level, read-only"""
    rng = np.random.default_rng(700 + level)
    n = eu.cell_size(level)
    src, mu = rng.uniform(-1.0, 1.0, (3, n)), rng.uniform(0.5, 50.0, n)
    ref = eu.apply_cell(src, mu, TET, level)
    for a in (src, mu, ref):
        a.setflags(write=False)
    return src, mu, ref


def check(got, expected, sel, filled):
    """per component: selected entries against the restatement, the others against the sentinel, bit by bit.  sel: one boolean
    array for all components, or one per component"""
    sel = np.broadcast_to(sel, got.shape)
    for c in range(3):
        g, e, s = got[c], expected[c], sel[c]
        assert np.array_equal(g[~s], filled[c][~s]), f"component {c}: entries outside the mask were written"
        scale = np.abs(e[s]).max() if s.any() else 0.0
        if scale == 0.0:
            assert np.array_equal(g[s], e[s])
            continue
        err = np.abs(g[s] - e[s])
        assert err.max() <= TOL * scale, (c, err.max(), scale)
        assert np.linalg.norm(err) <= TOL * np.linalg.norm(e[s]), c


def run_apply(torch, capi, level, mask, update):
    src, mu, ref = case(level)
    n = src.shape[1]
    filled = sentinel(n)
    (dt, dp), (st, sp), m = dev3(torch, filled), dev3(torch, src), dev(torch, mu)
    capi.p1_elementwise_epsilon_apply_macro_3d_masked(dp, sp, m.data_ptr(), TET, 1 << level, mask, update)
    torch.cuda.synchronize()
    if isinstance(mask, tuple):
        sel = np.stack([eu.point_mask(level, k) for k in mask])
    else:
        sel = eu.point_mask(level, mask)
    check(host3(dt), ref + filled if update == capi.ADD else ref, sel, filled)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("update", ["replace", "add"])
@pytest.mark.parametrize("level", range(8))
def test_apply_masked(env, level, update, mask):
    """level 2 has one inner point, 3 is the first with interior rows of unequal length, at 6 (7) an inner row spans two (three)
    62-lane segments; 0 and 1 use the point kernel only"""
    torch, capi = env
    run_apply(torch, capi, level, MASKS[mask], capi.ADD if update == "add" else capi.REPLACE)


@pytest.mark.parametrize("slot", range(14))
def test_apply_each_shell_class_alone(env, slot):
    """edge0..5, face0..3, vertex0..3 one at a time at level 3 (Replace) and level 1 (Add, the point kernel only)"""
    torch, capi = env
    run_apply(torch, capi, 3, 1 << slot, capi.REPLACE)
    run_apply(torch, capi, 1, 1 << slot, capi.ADD)


@pytest.mark.parametrize("level", [1, 3, 6])
def test_apply_with_a_mask_per_component(env, level):
    """a point that a component's mask excludes is not written in that component"""
    torch, capi = env
    run_apply(torch, capi, level, (eu.MASK_ALL, eu.MASK_INNER | (1 << 7), eu.MASK_SHELL), capi.REPLACE)
    run_apply(torch, capi, level, (1 << 4, 0, eu.MASK_INNER), capi.ADD)


def test_apply_level8(env):
    """level 8 has a brick shape of its own; every entry is compared"""
    torch, capi = env
    run_apply(torch, capi, 8, eu.MASK_ALL, capi.REPLACE)


def jacobi_inputs(level, seed):
    rng = np.random.default_rng(seed + level)
    n = eu.cell_size(level)
    return rng.uniform(-1.0, 1.0, (3, n)), rng.uniform(0.5, 2.0, (3, n))


@pytest.mark.parametrize("level", range(2, 8))
def test_fused_jacobi_step(env, level):
    """dst_i = src_i + omega * inv_diag_i .* ( rhs_i - ( A src )_i ) at the inner points, nothing else written"""
    torch, capi = env
    src, mu, ref = case(level)
    n = src.shape[1]
    rhs, invd = jacobi_inputs(level, 800)
    filled = sentinel(n)
    (dt, dp), (st, sp), (rt, rp), (it, ip), m = dev3(torch, filled), dev3(torch, src), dev3(torch, rhs), dev3(torch, invd), dev(torch, mu)
    capi.p1_elementwise_epsilon_jacobi_macro_3d(dp, sp, rp, ip, m.data_ptr(), TET, 1 << level, OMEGA)
    torch.cuda.synchronize()
    check(host3(dt), src + OMEGA * (invd * (rhs - ref)), eu.point_mask(level, eu.MASK_INNER), filled)


@pytest.mark.parametrize("level", range(8))
def test_diagonals(env, level):
    """diag_i += sum over the adjacent micro-cells of mean_mu A_e^{ii}[a][a], at all points"""
    torch, capi = env
    _, mu, _ = case(level)
    n = len(mu)
    filled = sentinel(n)
    (dt, dp), m = dev3(torch, filled), dev(torch, mu)
    capi.p1_elementwise_epsilon_diagonal_macro_3d(dp, m.data_ptr(), TET, 1 << level)
    torch.cuda.synchronize()
    check(host3(dt), filled + eu.diagonal_cell(mu, TET, level), np.ones(n, dtype=bool), filled)


def test_every_brick_shape_gives_the_same_bits(env):
    """the compiled brick shapes of the inner-point kernel at level 6 (several bricks per row with every shape)"""
    torch, capi = env
    level = 6
    src, mu, ref = case(level)
    n = src.shape[1]
    (st, sp), m = dev3(torch, src), dev(torch, mu)
    out = []
    try:
        for ny, lz in ((0, 0),) + tuple(capi.EPSILON_SHAPES):
            capi.p1_elementwise_epsilon_set_shape(ny, lz)
            dt, dp = dev3(torch, sentinel(n))
            capi.p1_elementwise_epsilon_apply_macro_3d_masked(dp, sp, m.data_ptr(), TET, 1 << level, eu.MASK_INNER, capi.REPLACE)
            torch.cuda.synchronize()
            out.append(host3(dt))
    finally:
        capi.p1_elementwise_epsilon_set_shape(0, 0)
    check(out[0], ref, eu.point_mask(level, eu.MASK_INNER), sentinel(n))
    for o in out[1:]:
        assert np.array_equal(o, out[0])


@pytest.mark.parametrize("level", [2, 5])
def test_inner_points_by_the_point_kernel(env, level):
    """the one-thread-per-point form of the inner points (the second implementation) computes the same operator, at the parity bar
    against the restatement and against the z-march"""
    torch, capi = env
    src, mu, ref = case(level)
    n = src.shape[1]
    rhs, invd = jacobi_inputs(level, 900)
    filled = sentinel(n)
    (st, sp), (rt, rp), (it, ip), m = dev3(torch, src), dev3(torch, rhs), dev3(torch, invd), dev(torch, mu)
    sel = eu.point_mask(level, eu.MASK_INNER)
    zt, zp = dev3(torch, filled)
    capi.p1_elementwise_epsilon_apply_macro_3d_masked(zp, sp, m.data_ptr(), TET, 1 << level, eu.MASK_INNER, capi.REPLACE)
    torch.cuda.synchronize()
    zmarch = host3(zt)
    try:
        capi.p1_elementwise_epsilon_set_inner_by_points(True)
        for update in (capi.REPLACE, capi.ADD):
            dt, dp = dev3(torch, filled)
            capi.p1_elementwise_epsilon_apply_macro_3d_masked(dp, sp, m.data_ptr(), TET, 1 << level, eu.MASK_INNER, update)
            torch.cuda.synchronize()
            check(host3(dt), ref + filled if update == capi.ADD else ref, sel, filled)
            if update == capi.REPLACE:
                check(host3(dt), zmarch, sel, filled)
        dt, dp = dev3(torch, filled)
        capi.p1_elementwise_epsilon_jacobi_macro_3d(dp, sp, rp, ip, m.data_ptr(), TET, 1 << level, OMEGA)
        torch.cuda.synchronize()
        check(host3(dt), src + OMEGA * (invd * (rhs - ref)), sel, filled)
    finally:
        capi.p1_elementwise_epsilon_set_inner_by_points(False)


@pytest.mark.parametrize("level", [4, 6])
def test_rigid_motion_gives_zero_at_inner_points(env, level):
    """a + b x X is in the kernel of every inner row for any mu: inner output <= 1e-12 * max mu * max|weight| * max|u|"""
    torch, capi = env
    _, mu, _ = case(level)
    n = len(mu)
    X = eu.cell_points(TET, level)
    a, b = np.array([0.3, -1.1, 0.7]), np.array([0.9, 0.4, -0.6])
    u = (a[None, :] + np.cross(b[None, :], X)).T
    (dt, dp), (st, sp), m = dev3(torch, sentinel(n)), dev3(torch, u), dev(torch, mu)
    capi.p1_elementwise_epsilon_apply_macro_3d_masked(dp, sp, m.data_ptr(), TET, 1 << level, eu.MASK_INNER, capi.REPLACE)
    torch.cuda.synchronize()
    inner = eu.point_mask(level, eu.MASK_INNER)
    bound = 1e-12 * mu.max() * eu.max_weight(TET, level) * np.abs(u).max()
    got = host3(dt)[:, inner]
    print(f"level {level}: max inner output {np.abs(got).max():.3e}, bound {bound:.3e}")
    assert np.abs(got).max() <= bound
