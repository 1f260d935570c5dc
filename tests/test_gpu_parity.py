"""GPU parity tests: every kernel is called through the C-ABI (hyteg_amd.capi -> libhyteg_hip.so) on
seeded inputs and compared with the CPU oracle.  Tolerance: relative L2 <= 1e-13 (north_star asks for
1e-12 for fp64); index/ownership properties (which entries a kernel may touch) are checked exactly."""
import numpy as np
import pytest

from conftest import OCT_TET, REF_TET, SKEW_TET

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi
    from oracle import p1_oracle as po

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    capi.lib()  # must load: no fallback
    return torch, capi, po


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("level", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("tet", [REF_TET, OCT_TET, SKEW_TET])
def test_apply_replace_and_add(env, level, tet):
    torch, capi, po = env
    rng = np.random.default_rng(100 + level)
    w = po.assemble_cell_stencil(tet, level)
    n = po.cell_size(level)
    src_h, dst0_h = rng.random(n), rng.random(n)
    src = _dev(torch, src_h)
    for update in (capi.REPLACE, capi.ADD):
        dst = _dev(torch, dst0_h)
        capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, update, _stream(torch))
        torch.cuda.synchronize()
        ref = dst0_h.copy()
        po.apply_cell(ref, src_h, level, w, update)
        got = dst.cpu().numpy()
        m = po.inner_mask(level)
        assert np.array_equal(got[~m], dst0_h[~m]), "boundary entries must not be written"
        assert _rel(got[m], ref[m]) < TOL


COMPILED_SHAPES = [(2, 8, 1), (4, 8, 2), (4, 8, 1), (4, 4, 2), (4, 4, 1), (2, 4, 1), (8, 4, 2)]  # HYTEG_ZM_SHAPES of p1_apply.hip


@pytest.mark.parametrize("level", [3, 6, 8])
def test_every_compiled_brick_shape_gives_the_same_bits(env, level):
    """hyteg_hip_set_apply_shape changes the work split between waves, not the arithmetic of a point: apply (Replace, Add),
    fused Jacobi and the residual are bit-identical for every shape compiled in (and equal to the oracle: the tests above
    run the default shapes)"""
    torch, capi, po = env
    rng = np.random.default_rng(7 + level)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    src, rhs, dst0 = (_dev(torch, rng.random(n)) for _ in range(3))
    st = _stream(torch)

    def run_all():
        out = []
        for update in (capi.REPLACE, capi.ADD):
            d = dst0.clone()
            capi.p1_apply_cell(d.data_ptr(), src.data_ptr(), level, w, update, st)
            out.append(d)
        d = dst0.clone()
        capi.p1_jacobi_cell(d.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, 0.7, None, st)
        out.append(d)
        d = dst0.clone()
        capi.p1_residual_cell(d.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, st)
        out.append(d)
        sf, rf, df = src.float(), rhs.float(), dst0.float()
        capi.p1_jacobi_cell_f32(df.data_ptr(), rf.data_ptr(), sf.data_ptr(), level, w, 0.7, None, st)
        out.append(df)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    try:
        ref = run_all()
        for shape in COMPILED_SHAPES:
            capi.set_apply_shape(*shape)
            got = run_all()
            for a, b in zip(got, ref):
                assert np.array_equal(a, b), f"shape {shape} differs from the default shape at level {level}"
        with pytest.raises(capi.HytegHipError, match="not compiled in"):
            capi.set_apply_shape(3, 7, 1)
    finally:
        capi.set_apply_shape()


def test_apply_random_weights_and_unaligned_source(env):
    """Non-symmetric random weights catch swapped stencil slots; the source pointer is only 8-byte aligned: the base of the
    z-march kernel's buffer addressing at these levels.  (The scalar staging path of the LDS-tiled kernel, which an 8-byte aligned
    source selects at level 11, is tested in test_gpu_level11_paths.py.)"""
    torch, capi, po = env
    rng = np.random.default_rng(5)
    for level in (3, 5, 6):
        w = rng.standard_normal(15)
        n = po.cell_size(level)
        buf_h = rng.random(n + 1)
        buf = _dev(torch, buf_h)
        src = buf[1:]  # 8-byte aligned only
        assert src.data_ptr() % 16 == 8
        dst = torch.zeros(n, dtype=torch.float64, device="cuda")
        capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.REPLACE, _stream(torch))
        torch.cuda.synchronize()
        ref = np.zeros(n)
        po.apply_cell(ref, np.ascontiguousarray(buf_h[1:]), level, w)
        assert _rel(dst.cpu().numpy(), ref) < TOL


def test_apply_level8_full_size_against_oracle_and_properties(env):
    """BASELINE config 2 size (tet(257) = 2,862,209 entries): direct comparison (the C oracle needs ~50 ms),
    plus the reference's own property: Laplace annihilates constants and linears
    (tests/hyteg/P1/P1LaplaceOperator3DTest.cpp:48,109-126, limit 2.8e-13) and linearity."""
    torch, capi, po = env
    level = 8
    n = po.cell_size(level)
    assert n == 2862209
    rng = np.random.default_rng(42)
    w = po.assemble_cell_stencil(REF_TET, level)
    src_h = rng.random(n)
    src = _dev(torch, src_h)
    dst = torch.zeros(n, dtype=torch.float64, device="cuda")
    capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.REPLACE, _stream(torch))
    torch.cuda.synchronize()
    ref = np.zeros(n)
    po.apply_cell(ref, src_h, level, w)
    got = dst.cpu().numpy()
    assert _rel(got, ref) < TOL
    assert int(np.count_nonzero(got)) <= po.cell_inner_size(level)
    # property: A(linear) = 0
    npts = po.cell_inner_size(level)
    for fn in (lambda x, y, z: 0 * x + 1.0, lambda x, y, z: 42 * x + y + 1337 * z):
        u = _dev(torch, po.interpolate(SKEW_TET, level, fn))
        ws = po.assemble_cell_stencil(SKEW_TET, level)
        r = torch.zeros(n, dtype=torch.float64, device="cuda")
        capi.p1_apply_cell(r.data_ptr(), u.data_ptr(), level, ws, capi.REPLACE, _stream(torch))
        torch.cuda.synchronize()
        assert float(torch.sqrt((r * r).sum() / npts)) < 2.8e-13
    # linearity: A(2u - 3v) == 2Au - 3Av
    v = _dev(torch, rng.random(n))
    comb = 2.0 * src - 3.0 * v
    r1 = torch.zeros_like(src)
    r2 = torch.zeros_like(src)
    r3 = torch.zeros_like(src)
    capi.p1_apply_cell(r1.data_ptr(), comb.data_ptr(), level, w, capi.REPLACE, _stream(torch))
    capi.p1_apply_cell(r2.data_ptr(), src.data_ptr(), level, w, capi.REPLACE, _stream(torch))
    capi.p1_apply_cell(r3.data_ptr(), v.data_ptr(), level, w, capi.REPLACE, _stream(torch))
    torch.cuda.synchronize()
    assert float(torch.linalg.norm(r1 - (2 * r2 - 3 * r3)) / torch.linalg.norm(r1)) < 1e-12


@pytest.mark.parametrize("level", [2, 3, 5, 6])
def test_jacobi_fused_matches_reference_composition(env, level):
    torch, capi, po = env
    rng = np.random.default_rng(7 + level)
    w = po.assemble_cell_stencil(OCT_TET, level)
    n = po.cell_size(level)
    src_h, rhs_h, dst0_h = rng.random(n), rng.random(n), rng.random(n)
    src, rhs = _dev(torch, src_h), _dev(torch, rhs_h)
    ref = dst0_h.copy()
    po.jacobi_cell(ref, rhs_h, src_h, level, w, 2.0 / 3.0)
    m = po.inner_mask(level)
    # constant inverse diagonal (NULL) and explicit inverse-diagonal function
    invd_h = rng.random(n) + 0.5
    for invd in (None, invd_h):
        dst = _dev(torch, dst0_h)
        if invd is None:
            capi.p1_jacobi_cell(dst.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, 2.0 / 3.0, None, _stream(torch))
            expect = ref
        else:
            invd_d = _dev(torch, invd)
            capi.p1_jacobi_cell(dst.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, 2.0 / 3.0, invd_d.data_ptr(),
                                _stream(torch))
            expect = dst0_h.copy()
            po.jacobi_cell(expect, rhs_h, src_h, level, w, 2.0 / 3.0, invdiag=invd)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[~m], dst0_h[~m])
        assert _rel(got[m], expect[m]) < TOL


def test_jacobi_level8(env):
    torch, capi, po = env
    level = 8
    rng = np.random.default_rng(8)
    w = po.assemble_cell_stencil(REF_TET, level)
    n = po.cell_size(level)
    src_h, rhs_h = rng.random(n), rng.random(n)
    dst = torch.zeros(n, dtype=torch.float64, device="cuda")
    src, rhs = _dev(torch, src_h), _dev(torch, rhs_h)
    capi.p1_jacobi_cell(dst.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, 0.6, None, _stream(torch))
    torch.cuda.synchronize()
    ref = np.zeros(n)
    po.jacobi_cell(ref, rhs_h, src_h, level, w, 0.6)
    assert _rel(dst.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("level", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("relax,backwards", [(1.0, False), (1.0, True), (0.3, False), (1.3, True)])
def test_sor_sweeps_reproduce_the_sequential_order(env, level, relax, backwards):
    """The hyperplane schedule must give the same values as the reference's sequential (z,y,x) sweep:
    any ordering mistake changes results at O(1), far above the tolerance."""
    torch, capi, po = env
    rng = np.random.default_rng(31 * level + int(relax * 10) + backwards)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    u_h, rhs_h = rng.random(n), rng.random(n)
    u, rhs = _dev(torch, u_h), _dev(torch, rhs_h)
    for _ in range(2):  # two consecutive sweeps
        capi.p1_sor_cell(u.data_ptr(), rhs.data_ptr(), level, w, relax, backwards, _stream(torch))
    torch.cuda.synchronize()
    ref = u_h.copy()
    for _ in range(2):
        po.sor_cell(ref, rhs_h, level, w, relax, backwards)
    got = u.cpu().numpy()
    m = po.inner_mask(level)
    assert np.array_equal(got[~m], u_h[~m])
    assert _rel(got[m], ref[m]) < 1e-12


def test_gauss_seidel_level7_vs_oracle(env):
    torch, capi, po = env
    level = 7
    rng = np.random.default_rng(77)
    w = po.assemble_cell_stencil(OCT_TET, level)
    n = po.cell_size(level)
    u_h, rhs_h = rng.random(n), rng.random(n)
    u, rhs = _dev(torch, u_h), _dev(torch, rhs_h)
    capi.p1_sor_cell(u.data_ptr(), rhs.data_ptr(), level, w, 1.0, False, _stream(torch))
    torch.cuda.synchronize()
    ref = u_h.copy()
    po.gs_cell(ref, rhs_h, level, w)
    assert _rel(u.cpu().numpy(), ref) < 1e-12


@pytest.mark.parametrize("relax,backwards", [(1.0, False), (0.7, True)])
def test_sor_level8_default_form_vs_the_sequential_oracle(env, relax, backwards):
    """VERDICT r01 / ADVICE: the blocked 16^3 form is the default from level 5 up and the headline level is 8 -- compare it there
    directly with the sequential (z,y,x) sweep of the oracle (fast=False: strict order, no contraction), forwards and backwards.
    The blocked form is order-exact in its updates but sums each update in three partial chains: 1e-12, not bit for bit."""
    torch, capi, po = env
    level = 8
    rng = np.random.default_rng(88 + backwards)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    u_h, rhs_h = rng.random(n), rng.random(n) * w[7]
    u, rhs = _dev(torch, u_h), _dev(torch, rhs_h)
    capi.p1_sor_cell(u.data_ptr(), rhs.data_ptr(), level, w, relax, backwards, _stream(torch))
    torch.cuda.synchronize()
    ref = u_h.copy()
    po.sor_cell(ref, rhs_h, level, w, relax, backwards, fast=False)
    assert _rel(u.cpu().numpy(), ref) < 1e-12


@pytest.mark.parametrize("level", [2, 4, 7, 8])
def test_residual_in_one_launch_has_the_bits_of_apply_and_assign(env, level):
    """hyteg_hip_p1_residual_cell: rhs - A src formed by the interior kernel = apply followed by assign( { 1, -1 }, { rhs, A src } )
    (the two steps of GeometricMultigridSolver.hpp:240-246), bit for bit, and both equal the oracle's apply to 1e-13."""
    torch, capi, po = env
    rng = np.random.default_rng(900 + level)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    x_h, b_h = rng.random(n), rng.random(n)
    x, b = _dev(torch, x_h), _dev(torch, b_h)
    two = _dev(torch, np.full(n, 7.0))
    one = _dev(torch, np.full(n, 7.0))
    capi.p1_apply_cell(two.data_ptr(), x.data_ptr(), level, w, 0, _stream(torch))
    capi.p1_assign_cell(two.data_ptr(), [1.0, -1.0], [b.data_ptr(), two.data_ptr()], level, _stream(torch))
    capi.p1_residual_cell(one.data_ptr(), b.data_ptr(), x.data_ptr(), level, w, _stream(torch))
    torch.cuda.synchronize()
    assert torch.equal(one, two)  # boundary entries untouched (7.0) in both
    ax = np.zeros(n)
    po.apply_cell(ax, x_h, level, w, po.REPLACE)
    inner = po.inner_mask(level)
    assert _rel(one.cpu().numpy()[inner], (b_h - ax)[inner]) < 1e-13


@pytest.mark.parametrize("level,nsweeps,relax,backwards", [(5, 3, 1.0, False), (6, 2, 1.0, True), (7, 3, 0.8, False), (8, 3, 1.0, False),
                                                             (8, 4, 1.3, True), (4, 3, 1.0, False)])
def test_pipelined_sweeps_equal_consecutive_sweeps_bit_for_bit(env, level, nsweeps, relax, backwards):
    """hyteg_hip_p1_sor_cell_sweeps: n sweeps as one pipeline of block wavefronts (sweep s + 1 four wavefronts behind sweep s) must
    give exactly the bits of n calls of hyteg_hip_p1_sor_cell, which the tests above compare with the sequential oracle
    (level 4: no pipeline, the entry point loops)."""
    torch, capi, po = env
    rng = np.random.default_rng(500 + level + nsweeps)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    u_h, rhs_h = rng.random(n), rng.random(n) * w[7]
    a, b, rhs = _dev(torch, u_h), _dev(torch, u_h), _dev(torch, rhs_h)
    for _ in range(nsweeps):
        capi.p1_sor_cell(a.data_ptr(), rhs.data_ptr(), level, w, relax, backwards, _stream(torch))
    capi.p1_sor_cell_sweeps(b.data_ptr(), rhs.data_ptr(), level, w, relax, nsweeps, backwards, _stream(torch))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    if level <= 6:  # and directly against the sequential oracle
        ref = u_h.copy()
        for _ in range(nsweeps):
            po.sor_cell(ref, rhs_h, level, w, relax, backwards, fast=False)
        assert _rel(b.cpu().numpy(), ref) < 1e-12


@pytest.mark.parametrize("level", [2, 4, 6])
def test_vector_kernels(env, level):
    torch, capi, po = env
    rng = np.random.default_rng(level)
    n = po.cell_size(level)
    hs = [rng.random(n) for _ in range(4)]
    ds = [_dev(torch, h) for h in hs]
    m = po.inner_mask(level)
    d0 = rng.random(n)
    for k in (1, 2, 3, 4):
        scal = list(rng.standard_normal(k))
        # assign
        dst = _dev(torch, d0)
        capi.p1_assign_cell(dst.data_ptr(), scal, [d.data_ptr() for d in ds[:k]], level, _stream(torch))
        torch.cuda.synchronize()
        ref = d0.copy()
        po.assign(ref, scal, hs[:k], level)
        got = dst.cpu().numpy()
        assert np.array_equal(got[~m], d0[~m]) and _rel(got[m], ref[m]) < TOL
        # add
        dst = _dev(torch, d0)
        capi.p1_add_cell(dst.data_ptr(), scal, [d.data_ptr() for d in ds[:k]], level, _stream(torch))
        torch.cuda.synchronize()
        ref = d0.copy()
        po.add(ref, scal, hs[:k], level)
        got = dst.cpu().numpy()
        assert np.array_equal(got[~m], d0[~m]) and _rel(got[m], ref[m]) < TOL
        # multElementwise
        dst = _dev(torch, d0)
        capi.p1_mult_cell(dst.data_ptr(), [d.data_ptr() for d in ds[:k]], level, _stream(torch))
        torch.cuda.synchronize()
        ref = d0.copy()
        po.mult_elementwise(ref, hs[:k], level)
        got = dst.cpu().numpy()
        assert np.array_equal(got[~m], d0[~m]) and _rel(got[m], ref[m]) < TOL
    # in-place forms used by smooth_jac: dst appears among the sources (P1Operator.hpp:441-445)
    dst = _dev(torch, d0)
    capi.p1_assign_cell(dst.data_ptr(), [1.0, -1.0], [ds[0].data_ptr(), dst.data_ptr()], level, _stream(torch))
    torch.cuda.synchronize()
    ref = d0.copy()
    po.assign(ref, [1.0, -1.0], [hs[0], ref], level)
    assert _rel(dst.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("level", [2, 5, 8])
def test_dot(env, level):
    torch, capi, po = env
    rng = np.random.default_rng(level)
    n = po.cell_size(level)
    a_h, b_h = rng.standard_normal(n), rng.standard_normal(n)
    a, b = _dev(torch, a_h), _dev(torch, b_h)
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    capi.p1_dot_cell(a.data_ptr(), b.data_ptr(), level, res.data_ptr(), ws.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    ref = po.dot(a_h, b_h, level)
    m = po.inner_mask(level)
    scale = float(np.abs(a_h[m] * b_h[m]).sum())
    assert abs(float(res[0]) - ref) < 1e-13 * scale
    # run-to-run determinism (fixed reduction order)
    res2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    capi.p1_dot_cell(a.data_ptr(), b.data_ptr(), level, res2.data_ptr(), ws.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert float(res2[0]) == float(res[0])


_NNC_MIXED = [3, 4, 5, 6, 7, 8, 2, 1, 2, 2, 9, 10, 11, 12]


@pytest.mark.parametrize("coarse_level", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("nnc", [[1] * 14, _NNC_MIXED])
def test_restrict(env, coarse_level, nnc):
    torch, capi, po = env
    rng = np.random.default_rng(coarse_level)
    fine_h = rng.random(po.cell_size(coarse_level + 1))
    fine = _dev(torch, fine_h)
    coarse = torch.full((po.cell_size(coarse_level),), -7.0, dtype=torch.float64, device="cuda")
    capi.p1_restrict_cell(coarse.data_ptr(), fine.data_ptr(), coarse_level, nnc, _stream(torch))
    torch.cuda.synchronize()
    ref = np.zeros(po.cell_size(coarse_level))
    po.restrict_cell(ref, fine_h, coarse_level, np.array(nnc, dtype=np.float64))
    assert _rel(coarse.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("coarse_level", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("nnc", [[1] * 14, _NNC_MIXED])
@pytest.mark.parametrize("update", [0, 1])
def test_prolongate_gather_equals_reference_scatter(env, coarse_level, nnc, update):
    torch, capi, po = env
    rng = np.random.default_rng(10 + coarse_level)
    coarse_h = rng.random(po.cell_size(coarse_level))
    fine0_h = rng.random(po.cell_size(coarse_level + 1))
    coarse, fine = _dev(torch, coarse_h), _dev(torch, fine0_h)
    capi.p1_prolongate_cell(coarse.data_ptr(), fine.data_ptr(), coarse_level, nnc, update, _stream(torch))
    torch.cuda.synchronize()
    ref = fine0_h.copy()
    po.prolongate_prepare(ref, coarse_level + 1, update)
    po.prolongate_cell(coarse_h, ref, coarse_level, np.array(nnc, dtype=np.float64))
    got = fine.cpu().numpy()
    assert _rel(got, ref) < TOL


def test_transfer_level7_to_8(env):
    """Full-size grid transfer: prolongation reproduces linears exactly
    (tests/hyteg/vertexdofspace/VertexDoFLinearProlongation3DTest.cpp:49,107-137) and <R f, c> == <f, P c>."""
    torch, capi, po = env
    lc = 7
    ones = [1] * 14
    fn = lambda x, y, z: 42 * x + y + 3 * z  # noqa: E731
    uc = _dev(torch, po.interpolate(OCT_TET, lc, fn))
    uf = torch.zeros(po.cell_size(lc + 1), dtype=torch.float64, device="cuda")
    capi.p1_prolongate_cell(uc.data_ptr(), uf.data_ptr(), lc, ones, capi.REPLACE, _stream(torch))
    torch.cuda.synchronize()
    exact = po.interpolate(OCT_TET, lc + 1, fn)
    assert np.abs(uf.cpu().numpy() - exact).max() < 1e-12
    rng = np.random.default_rng(3)
    f_h, c_h = rng.random(po.cell_size(lc + 1)), rng.random(po.cell_size(lc))
    f, c = _dev(torch, f_h), _dev(torch, c_h)
    Rf = torch.zeros(po.cell_size(lc), dtype=torch.float64, device="cuda")
    Pc = torch.zeros(po.cell_size(lc + 1), dtype=torch.float64, device="cuda")
    capi.p1_restrict_cell(Rf.data_ptr(), f.data_ptr(), lc, ones, _stream(torch))
    capi.p1_prolongate_cell(c.data_ptr(), Pc.data_ptr(), lc, ones, capi.REPLACE, _stream(torch))
    torch.cuda.synchronize()
    lhs, rhs = float(Rf @ c), float(f @ Pc)
    assert abs(lhs - rhs) < 1e-11 * abs(rhs)
    ref = np.zeros(po.cell_size(lc))
    po.restrict_cell(ref, f_h, lc, np.ones(14))
    assert _rel(Rf.cpu().numpy(), ref) < TOL


def test_kernels_run_on_a_side_stream(env):
    torch, capi, po = env
    level = 5
    rng = np.random.default_rng(1)
    w = po.assemble_cell_stencil(REF_TET, level)
    n = po.cell_size(level)
    src_h = rng.random(n)
    src = _dev(torch, src_h)
    dst = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.REPLACE, s.cuda_stream)
    s.synchronize()
    ref = np.zeros(n)
    po.apply_cell(ref, src_h, level, w)
    assert _rel(dst.cpu().numpy(), ref) < TOL
