"""GPU tests of the variable-coefficient diffusion kernels (include/hyteg_hip.h section b-4) through the C-ABI on one macro-cell,
entry by entry against the numpy element loop of tests/divkgradutil.py (pinned by tests/test_divkgrad_reference.py).
Criteria: relative L2 <= 1e-12 and max entry error <= 1e-12 * max|dst| (the project's fp64 parity bar); entries outside the class
mask are bit-identical to the sentinel the destination was filled with."""
import functools

import numpy as np
import pytest

import divkgradutil as dk
from conftest import SKEW_TET

pytestmark = pytest.mark.gpu
TOL = 1e-12
TET = SKEW_TET  # all six micro-cell types differ
MASKS = {"all": dk.MASK_ALL, "inner": dk.MASK_INNER, "shell": dk.MASK_SHELL, "face1": 1 << 7, "edge4": 1 << 4}


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi


def _dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")  # a copy: the shared cases are read-only arrays


def sentinel(n):
    return 7.0 + 3.0 * np.sin(0.37 * np.arange(n))


@functools.lru_cache(maxsize=None)
def case(level):
    """src in [-1, 1], k in [0.5, 2] and the restatement's ( A src ) on all points: computed once per level, read-only"""
    rng = np.random.default_rng(100 + level)
    n = dk.cell_size(level)
    src, k = rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n)
    ref = dk.apply_cell(src, k, TET, level)
    for a in (src, k, ref):
        a.setflags(write=False)
    return src, k, ref


def check(got, expected, sel, filled):
    """selected entries against the restatement, the others against the sentinel, bit by bit"""
    assert np.array_equal(got[~sel], filled[~sel]), "entries outside the mask were written"
    scale = np.abs(expected[sel]).max() if sel.any() else 0.0
    if scale == 0.0:
        assert np.array_equal(got[sel], expected[sel])
        return
    err = np.abs(got[sel] - expected[sel])
    assert err.max() <= TOL * scale, (err.max(), scale)
    assert np.linalg.norm(err) <= TOL * np.linalg.norm(expected[sel])


def run_apply(torch, capi, level, mask, update):
    src, k, ref = case(level)
    n = len(src)
    filled = sentinel(n)
    dst, s, kd = _dev(torch, filled), _dev(torch, src), _dev(torch, k)  # named: a temporary's memory is reused by the next upload
    capi.p1_elementwise_divkgrad_apply_macro_3d_masked(dst.data_ptr(), s.data_ptr(), kd.data_ptr(), TET, 1 << level, mask, update)
    torch.cuda.synchronize()
    sel = dk.point_mask(level, mask)
    check(dst.cpu().numpy(), ref + filled if update == capi.ADD else ref, sel, filled)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("update", ["replace", "add"])
@pytest.mark.parametrize("level", range(8))
def test_apply_masked(env, level, update, mask):
    """levels 6 and 7 are the first with more than one and more than two x-bricks per row"""
    torch, capi = env
    run_apply(torch, capi, level, MASKS[mask], capi.ADD if update == "add" else capi.REPLACE)


def test_apply_level8(env):
    """level 8 has a brick shape of its own; every entry is compared (the numpy element loop stays under the five seconds a test may take)"""
    torch, capi = env
    run_apply(torch, capi, 8, dk.MASK_ALL, capi.REPLACE)


@pytest.mark.parametrize("level", range(2, 8))
def test_fused_jacobi_step(env, level):
    """dst = src + omega * inv_diag .* ( rhs - A src ) at the inner points, nothing else written"""
    torch, capi = env
    src, k, ref = case(level)
    n = len(src)
    rng = np.random.default_rng(200 + level)
    rhs, invd, omega = rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n), 0.6
    filled = sentinel(n)
    dst, s, r, iv, kd = (_dev(torch, a) for a in (filled, src, rhs, invd, k))
    capi.p1_elementwise_divkgrad_jacobi_macro_3d(dst.data_ptr(), s.data_ptr(), r.data_ptr(), iv.data_ptr(), kd.data_ptr(), TET, 1 << level, omega)
    torch.cuda.synchronize()
    check(dst.cpu().numpy(), src + omega * (invd * (rhs - ref)), dk.point_mask(level, dk.MASK_INNER), filled)


@pytest.mark.parametrize("level", range(8))
def test_diagonal(env, level):
    """diag += sum over the adjacent micro-cells of mean_k K_e[i, i], at all points"""
    torch, capi = env
    _, k, _ = case(level)
    n = len(k)
    filled = sentinel(n)
    diag, kd = _dev(torch, filled), _dev(torch, k)
    capi.p1_elementwise_divkgrad_diagonal_macro_3d(diag.data_ptr(), kd.data_ptr(), TET, 1 << level)
    torch.cuda.synchronize()
    check(diag.cpu().numpy(), filled + dk.diagonal_cell(k, TET, level), np.ones(n, dtype=bool), filled)


@pytest.mark.parametrize("level", [1, 4, 6])
def test_constant_coefficient_is_a_multiple_of_the_laplacian(env, level):
    """k = c gives c times hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_masked, to 1e-13"""
    torch, capi = env
    src, _, _ = case(level)
    n, c = len(src), 2.75
    s = _dev(torch, src)
    a, b, kd = _dev(torch, np.zeros(n)), _dev(torch, np.zeros(n)), _dev(torch, np.full(n, c))
    capi.p1_elementwise_divkgrad_apply_macro_3d_masked(a.data_ptr(), s.data_ptr(), kd.data_ptr(), TET, 1 << level, dk.MASK_ALL, capi.REPLACE)
    capi.p1_elementwise_diffusion_apply_macro_3d_masked(b.data_ptr(), s.data_ptr(), TET, 1 << level, dk.MASK_ALL, capi.REPLACE)
    torch.cuda.synchronize()
    got, lap = a.cpu().numpy(), c * b.cpu().numpy()
    assert np.abs(got - lap).max() <= 1e-13 * np.abs(lap).max()
    assert np.linalg.norm(got - lap) <= 1e-13 * np.linalg.norm(lap)


@pytest.mark.parametrize("level", [1, 4, 6])
def test_constant_source_gives_zero(env, level):
    """the element matrices have zero row sums: src = const gives zero for any k, to 1e-12 of max|k| max|K_e|"""
    torch, capi = env
    _, k, _ = case(level)
    n = len(k)
    dst, s, kd = _dev(torch, sentinel(n)), _dev(torch, np.full(n, 1.7)), _dev(torch, k)
    capi.p1_elementwise_divkgrad_apply_macro_3d_masked(dst.data_ptr(), s.data_ptr(), kd.data_ptr(), TET, 1 << level, dk.MASK_ALL, capi.REPLACE)
    torch.cuda.synchronize()
    assert np.abs(dst.cpu().numpy()).max() <= 1e-12 * k.max() * dk.max_weight(TET, level)


def test_every_brick_shape_gives_the_same_bits(env):
    """the compiled brick shapes of the inner-point kernel at level 6 (several bricks per row with every shape)"""
    torch, capi = env
    level = 6
    src, k, ref = case(level)
    n = len(src)
    s, kd = _dev(torch, src), _dev(torch, k)
    out = []
    try:
        for ny, lz in capi.DIVKGRAD_SHAPES:
            capi.p1_elementwise_divkgrad_set_shape(ny, lz)
            dst = _dev(torch, sentinel(n))
            capi.p1_elementwise_divkgrad_apply_macro_3d_masked(dst.data_ptr(), s.data_ptr(), kd.data_ptr(), TET, 1 << level, dk.MASK_INNER,
                                                               capi.REPLACE)
            torch.cuda.synchronize()
            out.append(dst.cpu().numpy())
    finally:
        capi.p1_elementwise_divkgrad_set_shape(0, 0)
    check(out[0], ref, dk.point_mask(level, dk.MASK_INNER), sentinel(n))
    for o in out[1:]:
        assert np.array_equal(o, out[0])


@pytest.mark.parametrize("level", [2, 5])
def test_inner_points_by_the_point_kernel(env, level):
    """the one-thread-per-point form of the inner points (the measurement switch) computes the same operator"""
    torch, capi = env
    src, k, ref = case(level)
    n = len(src)
    rng = np.random.default_rng(300 + level)
    rhs, invd, omega = rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n), 0.6
    filled = sentinel(n)
    s, kd = _dev(torch, src), _dev(torch, k)
    sel = dk.point_mask(level, dk.MASK_INNER)
    try:
        capi.p1_elementwise_divkgrad_set_inner_by_points(True)
        for update in (capi.REPLACE, capi.ADD):
            dst = _dev(torch, filled)
            capi.p1_elementwise_divkgrad_apply_macro_3d_masked(dst.data_ptr(), s.data_ptr(), kd.data_ptr(), TET, 1 << level, dk.MASK_INNER, update)
            torch.cuda.synchronize()
            check(dst.cpu().numpy(), ref + filled if update == capi.ADD else ref, sel, filled)
        dst, r, iv = _dev(torch, filled), _dev(torch, rhs), _dev(torch, invd)
        capi.p1_elementwise_divkgrad_jacobi_macro_3d(dst.data_ptr(), s.data_ptr(), r.data_ptr(), iv.data_ptr(), kd.data_ptr(), TET, 1 << level, omega)
        torch.cuda.synchronize()
        check(dst.cpu().numpy(), src + omega * (invd * (rhs - ref)), sel, filled)
    finally:
        capi.p1_elementwise_divkgrad_set_inner_by_points(False)
