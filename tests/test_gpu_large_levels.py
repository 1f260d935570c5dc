"""The upper end of the supported level range (HYTEG_HIP_MAX_LEVEL = 11): the kernels switch index arithmetic and code
paths with the size -- 32-bit slice offsets up to level 10, 64-bit above; buffer addressing with a 32-bit byte range up to
level 8..10 arrays (23 MB .. 1.4 GB), the LDS-tiled apply with 64-bit pointers for the 11.5 GB arrays of level 11.
Level 9 is compared with the CPU oracle entry by entry for every kernel of the path; levels 10 and 11 check the apply against
a stencil evaluation at random points done with torch on the device (the arrays never leave the GPU) and against the
reference's own property that the Laplace stencil annihilates linear functions (P1LaplaceOperator3DTest.cpp:109-126)."""
import numpy as np
import pytest

from conftest import OCT_TET, SKEW_TET

pytestmark = pytest.mark.gpu

OFFS = [(0, 0, -1), (1, 0, -1), (-1, 1, -1), (0, 1, -1), (0, -1, 0), (1, -1, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (-1, 1, 0),
        (0, 1, 0), (0, -1, 1), (1, -1, 1), (-1, 0, 1), (0, 0, 1)]  # order of the 15 weights (include/hyteg_hip.h)


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi, po


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def test_level9_every_kernel_against_the_oracle(env):
    torch, capi, po = env
    level = 9
    n, nc = po.cell_size(level), po.cell_size(level - 1)
    assert n == 22632705
    rng = np.random.default_rng(9)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    a_h, b_h = rng.random(n), rng.random(n)
    a, b = torch.from_numpy(a_h).cuda(), torch.from_numpy(b_h).cuda()
    m = po.inner_mask(level)
    # apply Replace / Add
    d = torch.from_numpy(b_h).cuda()
    capi.p1_apply_cell(d.data_ptr(), a.data_ptr(), level, w, capi.ADD)
    ref = b_h.copy()
    po.apply_cell(ref, a_h, level, w, capi.ADD)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got[~m], b_h[~m])
    assert _rel(got[m], ref[m]) < 1e-13
    # fused Jacobi
    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    capi.p1_jacobi_cell(d.data_ptr(), b.data_ptr(), a.data_ptr(), level, w, 0.6, None)
    ref = np.zeros(n)
    po.jacobi_cell(ref, b_h, a_h, level, w, 0.6)
    torch.cuda.synchronize()
    assert _rel(d.cpu().numpy(), ref) < 1e-13
    # assign, dot
    capi.p1_assign_cell(d.data_ptr(), [2.0, -0.5], [a.data_ptr(), b.data_ptr()], level)
    torch.cuda.synchronize()
    assert _rel(d.cpu().numpy()[m], (2.0 * a_h - 0.5 * b_h)[m]) < 1e-15
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    capi.p1_dot_cell(a.data_ptr(), b.data_ptr(), level, res.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    assert abs(float(res[0]) - float(np.dot(a_h[m], b_h[m]))) < 1e-11 * float(np.dot(a_h[m], b_h[m]))
    # grid transfer 9 <-> 8
    nnc = [1.0] * 14
    coarse = torch.zeros(nc, dtype=torch.float64, device="cuda")
    capi.p1_restrict_cell(coarse.data_ptr(), a.data_ptr(), level - 1, nnc)
    ref = np.zeros(nc)
    po.restrict_cell(ref, a_h, level - 1, nnc)
    torch.cuda.synchronize()
    assert _rel(coarse.cpu().numpy(), ref) < 1e-13
    c_h = rng.random(nc)
    fine = torch.zeros(n, dtype=torch.float64, device="cuda")
    capi.p1_prolongate_cell(torch.from_numpy(c_h).cuda().data_ptr(), fine.data_ptr(), level - 1, nnc, capi.REPLACE)
    ref = np.zeros(n)
    po.prolongate_prepare(ref, level, capi.REPLACE)
    po.prolongate_cell(c_h, ref, level - 1, nnc)
    torch.cuda.synchronize()
    assert _rel(fine.cpu().numpy(), ref) < 1e-13
    # Gauss-Seidel, exact order (blocked form: 32 x 32 x 32 blocks of 16^3)
    u = torch.from_numpy(a_h).cuda()
    capi.p1_sor_cell(u.data_ptr(), b.data_ptr(), level, w, 1.0, False)
    ref = a_h.copy()
    po.sor_cell(ref, b_h, level, w, 1.0, False)
    torch.cuda.synchronize()
    assert _rel(u.cpu().numpy(), ref) < 1e-12


ROW_SLICES = (1, 2, 511, 1023)  # whole rows y = 1, 2 of these slices: at level 11 each is longer than a 1024-entry tile of the LDS-tiled kernel


def _sample_indices(torch, capi, level, nsamples, seed):
    """(centre, neighbours): int64 device tensors with the array index of the sampled interior points and of their 15 stencil
    neighbours (order of OFFS).  The sample: `nsamples` random interior points, the corners of the interior (first / last inner point
    of the array, longest row, tip), and every interior x of rows y = 1, 2 of the slices ROW_SLICES that the level has -- at level
    11 such a row crosses at least one tile seam wherever the tile table puts it, and only there a tile lies strictly inside one row"""
    N = (1 << level) + 1
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < nsamples:
        x, y, z = (int(v) for v in rng.integers(1, N - 2, 3))
        if x + y + z <= N - 2:
            pts.append((x, y, z))
    pts += [(1, 1, 1), (N - 4, 1, 1), (1, N - 4, 1), (1, 1, N - 4), (N - 5, 2, 1)]
    centre = [torch.tensor([capi.cell_index(level, *p) for p in pts], dtype=torch.int64, device="cuda")]
    nb = [[torch.tensor([capi.cell_index(level, x + dx, y + dy, z + dz) for x, y, z in pts], dtype=torch.int64, device="cuda")]
          for dx, dy, dz in OFFS]
    for z in ROW_SLICES:
        for y in (1, 2):
            if N - 2 - y - z < 1:
                continue
            x = torch.arange(1, N - 1 - y - z, dtype=torch.int64, device="cuda")  # interior x: 1 .. N - 2 - y - z
            centre.append(capi.cell_index(level, 0, y, z) + x)
            for k, (dx, dy, dz) in enumerate(OFFS):
                nb[k].append(capi.cell_index(level, 0, y + dy, z + dz) + x + dx)
    return torch.cat(centre), [torch.cat(t) for t in nb]


def _stencil_at(w, src, nb):
    """sum_k w[k] src[neighbour k] at the sampled points, with torch on the device"""
    au = w[0] * src[nb[0]]
    for k in range(1, 15):
        au += w[k] * src[nb[k]]
    return au


def _boundary_probes(capi, level):
    """entries no interior kernel writes: first and last array entries, the tip, two face points"""
    N = (1 << level) + 1
    return [capi.cell_index(level, *p) for p in ((0, 0, 0), (N - 1, 0, 0), (0, 0, N - 1), (3, 0, 5), (0, 4, 4))]


def _sampled_apply_check(torch, capi, po, level, nsamples=3000, mode="replace", unaligned=False):
    """apply / fused Jacobi on device arrays that never leave the GPU; the stencil is re-evaluated with torch at the points of
    _sample_indices.  mode: "replace", "add" (dst pre-filled with a second random array) or "jacobi_invdiag" (inverse-diagonal array);
    unaligned: the source starts one entry into its buffer (8-byte aligned: the scalar staging of the LDS-tiled kernel at level 11)"""
    n = capi.cell_size(level)
    N = (1 << level) + 1
    w = po.assemble_cell_stencil(OCT_TET, level)
    g = torch.Generator(device="cuda")
    g.manual_seed(level)
    buf = torch.rand(n + int(unaligned), dtype=torch.float64, device="cuda", generator=g)
    src = buf[1:] if unaligned else buf
    assert src.data_ptr() % 16 == (8 if unaligned else 0)
    centre, nb = _sample_indices(torch, capi, level, nsamples, seed=level)
    probes = _boundary_probes(capi, level)
    want = _stencil_at(w, src, nb)
    if mode == "replace":
        dst = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.REPLACE)
        before, bound = [7.0] * len(probes), 1e-13
    elif mode == "add":
        dst = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
        want += dst[centre]
        before = [float(dst[i]) for i in probes]
        capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.ADD)
        bound = 1e-13
    else:
        assert mode == "jacobi_invdiag"
        rhs = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
        inv = (0.5 + torch.rand(n, dtype=torch.float64, device="cuda", generator=g)) / w[7]
        want = src[centre] + 0.6 * (inv[centre] * (rhs[centre] - want))
        dst = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        capi.p1_jacobi_cell(dst.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, 0.6, inv.data_ptr())
        before, bound = [7.0] * len(probes), 1e-12
    torch.cuda.synchronize()
    got = dst[centre]
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"level {level} {mode}{' unaligned' if unaligned else ''}: {centre.numel()} points, largest error {err:.3e}, largest |want| {scale:.3e}")
    assert err <= bound * scale
    # boundary entries are not written
    for i, v in zip(probes, before):
        assert float(dst[i]) == v
    del dst
    return n, N, w, src


@pytest.mark.parametrize("level", [10, 11])
def test_apply_at_the_largest_levels(env, level):
    torch, capi, po = env
    free, _ = torch.cuda.mem_get_info()
    n = capi.cell_size(level)
    if free < 3.2 * n * 8:
        pytest.skip(f"needs {3.2 * n * 8 / 2**30:.0f} GiB of device memory")
    n, N, w, src = _sampled_apply_check(torch, capi, po, level)
    # Laplace of a linear function vanishes at every inner point (checked through the largest magnitude): fill src with
    # 3x - 2y + 5z + 1 using the array layout (index of (x,y,z) = slice start + row start + x)
    k = 0
    src.zero_()
    z_starts = [capi.cell_index(level, 0, 0, z) for z in range(N)]
    for z in range(N):
        W = N - z
        # rows of this slice: lengths W, W-1, ..., 1; coordinates from the slice-local offset
        j = torch.arange(W * (W + 1) // 2, dtype=torch.int64, device="cuda")
        # row y of offset j: largest y with y*W - y(y-1)/2 <= j
        y = torch.floor(((2 * W + 1) - torch.sqrt(((2 * W + 1) ** 2 - 8 * j).double())) / 2).long()
        y = torch.where(y * W - y * (y - 1) // 2 > j, y - 1, y)
        y = torch.where((y + 1) * W - (y + 1) * y // 2 <= j, y + 1, y)
        x = j - (y * W - y * (y - 1) // 2)
        src[z_starts[z]:z_starts[z] + j.numel()] = 3.0 * x.double() - 2.0 * y.double() + 5.0 * z + 1.0
    dst = torch.zeros(n, dtype=torch.float64, device="cuda")
    capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, capi.REPLACE)
    torch.cuda.synchronize()
    # |w| ~ 2^level-independent O(1) sums of values up to ~1e4: rounding level 1e-16 * 15 * 1e4
    assert float(dst.abs().max()) < 1e-9
    assert float(src[capi.cell_index(level, 2, 3, 4)]) == 3 * 2 - 2 * 3 + 5 * 4 + 1


def _inner_mask_on_device(torch, capi, level):
    """bool array: True at inner points (x, y, z >= 1, x + y + z <= N - 2), built slice by slice from the layout"""
    N = (1 << level) + 1
    n = capi.cell_size(level)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    for z in range(1, N - 2):
        W = N - z
        j = torch.arange(W * (W + 1) // 2, dtype=torch.int64, device="cuda")
        y = torch.floor(((2 * W + 1) - torch.sqrt(((2 * W + 1) ** 2 - 8 * j).double())) / 2).long()
        y = torch.where(y * W - y * (y - 1) // 2 > j, y - 1, y)
        y = torch.where((y + 1) * W - (y + 1) * y // 2 <= j, y + 1, y)
        x = j - (y * W - y * (y - 1) // 2)
        s0 = capi.cell_index(level, 0, 0, z)
        mask[s0:s0 + j.numel()] = (x >= 1) & (y >= 1) & (x + y + z <= N - 2)
    return mask


def test_vector_kernels_jacobi_and_transfer_at_level_11(env):
    """11.5 GB per array: every index of these kernels has to be 64-bit clean.  Checked on the device against torch."""
    torch, capi, po = env
    level = 11
    n = capi.cell_size(level)
    free, _ = torch.cuda.mem_get_info()
    if free < 6.5 * n * 8:
        pytest.skip(f"needs {6.5 * n * 8 / 2**30:.0f} GiB of device memory")
    N = (1 << level) + 1
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    a = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    mask = _inner_mask_on_device(torch, capi, level)
    assert int(mask.sum()) == capi.cell_inner_size(level)
    # assign: inner points get 2a - 0.5b, everything else keeps its value
    d = torch.full((n,), -3.0, dtype=torch.float64, device="cuda")
    capi.p1_assign_cell(d.data_ptr(), [2.0, -0.5], [a.data_ptr(), b.data_ptr()], level)
    torch.cuda.synchronize()
    want = torch.where(mask, 2.0 * a - 0.5 * b, torch.full_like(a, -3.0))
    assert bool(torch.equal(d, want))
    del want
    # dot over the inner points
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    capi.p1_dot_cell(a.data_ptr(), b.data_ptr(), level, res.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    ref = float((a * b * mask).sum())
    assert abs(float(res[0]) - ref) <= 1e-11 * ref
    # fused Jacobi at random points (and untouched boundary)
    w = po.assemble_cell_stencil(OCT_TET, level)
    d.fill_(-3.0)
    capi.p1_jacobi_cell(d.data_ptr(), b.data_ptr(), a.data_ptr(), level, w, 0.6, None)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    pts = []
    while len(pts) < 2000:
        x, y, z = (int(v) for v in rng.integers(1, N - 2, 3))
        if x + y + z <= N - 2:
            pts.append((x, y, z))
    pts += [(1, 1, 1), (N - 4, 1, 1), (1, N - 4, 1), (1, 1, N - 4)]
    centre = torch.tensor([capi.cell_index(level, *p) for p in pts], dtype=torch.int64, device="cuda")
    au = torch.zeros(len(pts), dtype=torch.float64, device="cuda")
    for k, (dx, dy, dz) in enumerate(OFFS):
        idx = torch.tensor([capi.cell_index(level, x + dx, y + dy, z + dz) for x, y, z in pts], dtype=torch.int64, device="cuda")
        au += w[k] * a[idx]
    want = a[centre] + 0.6 * (1.0 / w[7]) * (b[centre] - au)
    assert float((d[centre] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(d[capi.cell_index(level, 0, 5, 5)]) == -3.0 and float(d[n - 1]) == -3.0
    del d, mask
    # grid transfer 11 <-> 10 on constants: restriction of 1 with all neighbour counts 1 gives the column sums of the
    # prolongation (8 at inner coarse points: 1 + 14/2), prolongation of 1 gives 1 at every fine point
    nc = capi.cell_size(level - 1)
    a.fill_(1.0)
    coarse = torch.zeros(nc, dtype=torch.float64, device="cuda")
    capi.p1_restrict_cell(coarse.data_ptr(), a.data_ptr(), level - 1, [1.0] * 14)
    torch.cuda.synchronize()
    assert float(coarse[capi.cell_index(level - 1, 3, 4, 5)]) == 8.0
    assert float(coarse[capi.cell_index(level - 1, 1, 1, (1 << (level - 1)) - 3)]) == 8.0  # the last inner point along z
    assert float(coarse.max()) == 8.0
    coarse.fill_(1.0)
    b.fill_(-1.0)
    capi.p1_prolongate_cell(coarse.data_ptr(), b.data_ptr(), level - 1, [1.0] * 14, capi.REPLACE)
    torch.cuda.synchronize()
    assert float(b.min()) == 1.0 and float(b.max()) == 1.0


@pytest.mark.parametrize("mode,unaligned", [("add", False), ("jacobi_invdiag", False), ("replace", True)])
def test_apply_modes_and_scalar_staging_at_level_11(env, mode, unaligned):
    """what test_apply_at_the_largest_levels leaves out of the LDS-tiled kernel at 11.5 GB: Add, Jacobi with an inverse-diagonal
    array, and the scalar staging of an 8-byte aligned source (their arithmetic is compared entry by entry at levels 2..7 in
    test_gpu_level11_paths.py; here the addressing)"""
    torch, capi, po = env
    level = 11
    free, _ = torch.cuda.mem_get_info()
    n = capi.cell_size(level)
    arrays = {"add": 2, "jacobi_invdiag": 4, "replace": 2}[mode]
    if free < (arrays + 1.2) * n * 8:
        pytest.skip(f"needs {(arrays + 1.2) * n * 8 / 2**30:.0f} GiB of device memory")
    _sampled_apply_check(torch, capi, po, level, mode=mode, unaligned=unaligned)


def test_chebyshev_steps_at_level_11(env):
    """hyteg_hip_p1_chebyshev_start_cell / _step_cell at 11.5 GB per array (the steps composed from apply, assign, mult and add),
    inverse-diagonal array, has_prev = 1: against the stencil re-evaluated with torch at the points of _sample_indices"""
    torch, capi, po = env
    level = 11
    n = capi.cell_size(level)
    free, _ = torch.cuda.mem_get_info()
    if free < 6.5 * n * 8:
        pytest.skip(f"needs {6.5 * n * 8 / 2**30:.0f} GiB of device memory")
    w = po.assemble_cell_stencil(OCT_TET, level)
    g = torch.Generator(device="cuda")
    g.manual_seed(211)
    x, rhs = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
    inv = (0.5 + torch.rand(n, dtype=torch.float64, device="cuda", generator=g)) / w[7]
    t_out = torch.full((n,), -3.0, dtype=torch.float64, device="cuda")
    centre, nb = _sample_indices(torch, capi, level, 2000, seed=5)
    probes = _boundary_probes(capi, level)
    x_probes = [float(x[i]) for i in probes]
    # start: t_out = inv .* ( rhs - A x ), x untouched
    want = inv[centre] * (rhs[centre] - _stencil_at(w, x, nb))
    x_before = x[centre].clone()
    capi.p1_chebyshev_start_cell(t_out.data_ptr(), rhs.data_ptr(), x.data_ptr(), level, w, invdiag=inv.data_ptr())
    torch.cuda.synchronize()
    err, scale = float((t_out[centre] - want).abs().max()), float(want.abs().max())
    print(f"start t_out: {centre.numel()} points, largest error {err:.3e}, largest |want| {scale:.3e}")
    assert err <= 1e-12 * scale
    assert bool(torch.equal(x[centre], x_before))
    assert all(float(t_out[i]) == -3.0 for i in probes) and [float(x[i]) for i in probes] == x_probes
    # step: t_out = inv .* ( A t_in ); x = ( x + c_prev t_in ) + c_cur t_out, with rhs as t_in
    c_prev, c_cur = 0.8317, -0.2113
    t_in = rhs
    t_out.fill_(-3.0)
    want_t = inv[centre] * _stencil_at(w, t_in, nb)
    want_x = (x_before + c_prev * t_in[centre]) + c_cur * want_t
    capi.p1_chebyshev_step_cell(t_out.data_ptr(), x.data_ptr(), t_in.data_ptr(), level, w, c_prev, c_cur, has_prev=True, invdiag=inv.data_ptr())
    torch.cuda.synchronize()
    for what, got, wanted in (("step t_out", t_out[centre], want_t), ("step x", x[centre], want_x)):
        err, scale = float((got - wanted).abs().max()), float(wanted.abs().max())
        print(f"{what}: largest error {err:.3e}, largest |want| {scale:.3e}")
        assert err <= 1e-12 * scale
    assert all(float(t_out[i]) == -3.0 for i in probes) and [float(x[i]) for i in probes] == x_probes


def test_grid_transfer_level_10_to_11_on_a_linear_and_adjointness(env):
    """fine level 11 is the tile prolongation with 64-bit pointers: prolongation of a linear function in the index coordinates
    reproduces it at every fine point, and <R f, c> = <f, P c> for random f and c (all neighbour counts 1: P writes every fine
    entry, R every coarse one) -- an index error beyond 32 bits moves either by O(1)"""
    torch, capi, po = env
    lc, lf = 10, 11
    nc, nf = capi.cell_size(lc), capi.cell_size(lf)
    free, _ = torch.cuda.mem_get_info()
    if free < 4.5 * nf * 8:
        pytest.skip(f"needs {4.5 * nf * 8 / 2**30:.0f} GiB of device memory")
    ones = [1.0] * 14
    coarse = _linear(torch, lc)
    assert coarse.numel() == nc
    fine = torch.full((nf,), -1.0, dtype=torch.float64, device="cuda")
    capi.p1_prolongate_cell(coarse.data_ptr(), fine.data_ptr(), lc, ones, capi.REPLACE)
    torch.cuda.synchronize()
    want = _linear(torch, lf)
    assert want.numel() == nf
    scale = float(want.abs().max())
    want -= fine
    err = float(want.abs().max())
    del want
    print(f"prolongation of a linear function onto level {lf}: largest error {err:.3e}, largest |want| {scale:.3e}")
    assert err <= 1e-13 * scale
    g = torch.Generator(device="cuda")
    g.manual_seed(1011)
    f = torch.rand(nf, dtype=torch.float64, device="cuda", generator=g)
    c = torch.rand(nc, dtype=torch.float64, device="cuda", generator=g)
    Rf = torch.zeros(nc, dtype=torch.float64, device="cuda")
    capi.p1_restrict_cell(Rf.data_ptr(), f.data_ptr(), lc, ones)
    capi.p1_prolongate_cell(c.data_ptr(), fine.data_ptr(), lc, ones, capi.REPLACE)
    torch.cuda.synchronize()
    lhs = float((Rf * c).sum())
    f *= fine
    rhs = float(f.sum())
    print(f"<R f, c> = {lhs!r}, <f, P c> = {rhs!r}, relative difference {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-11 * abs(rhs)


def test_gauss_seidel_level_10_against_the_oracle(env):
    """180 M points, 64^3 / 6 blocks of 16^3 in 190 block wavefronts: block tables, row-base table and staging at 1.4 GB"""
    torch, capi, po = env
    level = 10
    n = po.cell_size(level)
    rng = np.random.default_rng(10)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    u_h, b_h = rng.random(n), rng.random(n)
    u, b = torch.from_numpy(u_h).cuda(), torch.from_numpy(b_h).cuda()
    capi.p1_sor_cell(u.data_ptr(), b.data_ptr(), level, w, 1.0, False)
    capi.p1_sor_cell(u.data_ptr(), b.data_ptr(), level, w, 1.2, True)
    po.sor_cell(u_h, b_h, level, w, 1.0, False)
    po.sor_cell(u_h, b_h, level, w, 1.2, True)
    torch.cuda.synchronize()
    assert _rel(u.cpu().numpy(), u_h) < 1e-12


def test_gauss_seidel_level_11_leaves_a_linear_function_alone(env):
    """A u = 0 for linear u, so with rhs = 0 every update of a sweep reproduces the value it replaces: a fixed point of the
    smoother whatever the order -- and any wrong index at 11.5 GB shows as a jump of O(1000)"""
    torch, capi, po = env
    level = 11
    n = capi.cell_size(level)
    free, _ = torch.cuda.mem_get_info()
    if free < 3.5 * n * 8:
        pytest.skip(f"needs {3.5 * n * 8 / 2**30:.0f} GiB of device memory")
    N = (1 << level) + 1
    w = po.assemble_cell_stencil(OCT_TET, level)
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    for z in range(N):
        W = N - z
        j = torch.arange(W * (W + 1) // 2, dtype=torch.int64, device="cuda")
        y = torch.floor(((2 * W + 1) - torch.sqrt(((2 * W + 1) ** 2 - 8 * j).double())) / 2).long()
        y = torch.where(y * W - y * (y - 1) // 2 > j, y - 1, y)
        y = torch.where((y + 1) * W - (y + 1) * y // 2 <= j, y + 1, y)
        x = j - (y * W - y * (y - 1) // 2)
        s0 = capi.cell_index(level, 0, 0, z)
        u[s0:s0 + j.numel()] = 3.0 * x.double() - 2.0 * y.double() + 5.0 * z + 1.0
    u0 = u.clone()
    rhs = torch.zeros(n, dtype=torch.float64, device="cuda")
    capi.p1_sor_cell(u.data_ptr(), rhs.data_ptr(), level, w, 1.0, False)
    capi.p1_sor_cell(u.data_ptr(), rhs.data_ptr(), level, w, 1.0, True)
    torch.cuda.synchronize()
    assert float((u - u0).abs().max()) < 1e-8  # values up to 1e4, 2 x 15-term sums per point


def _linear(torch, level):
    """3x - 2y + 5z in units of the level's mesh width, + 1: built slice by slice, row by row on the device"""
    N = (1 << level) + 1
    h = 1.0 / (N - 1)
    parts = []
    for z in range(N):
        W = N - z
        ys = torch.repeat_interleave(torch.arange(W, device="cuda"), torch.arange(W, 0, -1, device="cuda"))
        starts = torch.cumsum(torch.arange(W, 0, -1, device="cuda"), 0) - torch.arange(W, 0, -1, device="cuda")
        xs = torch.arange(ys.numel(), device="cuda") - starts[ys]
        parts.append((3.0 * xs - 2.0 * ys + 5.0 * z).to(torch.float64) * h + 1.0)
    return torch.cat(parts)


def test_grid_transfer_level_9_to_10_on_constants_and_a_linear(env):
    """fine level 10 (1.44 GB per array) is the largest level of the brick prolongation and of 32-bit buffer offsets: prolongation
    of 1 is 1 everywhere; prolongation of a linear function in the index coordinates reproduces it (P1 interpolation is exact
    for linears: VertexDoFLinearProlongation3DTest.cpp:107-137), checked at every fine point on the device; restriction of 1
    with all neighbour counts 1 gives 8 at inner coarse points."""
    torch, capi, po = env
    lc, lf = 9, 10
    nc, nf = capi.cell_size(lc), capi.cell_size(lf)
    free, _ = torch.cuda.mem_get_info()
    if free < 4.5 * nf * 8:
        pytest.skip(f"needs {4.5 * nf * 8 / 2**30:.0f} GiB of device memory")

    linear = lambda level: _linear(torch, level)  # noqa: E731
    ones = [1.0] * 14
    coarse = torch.ones(nc, dtype=torch.float64, device="cuda")
    fine = torch.full((nf,), -1.0, dtype=torch.float64, device="cuda")
    capi.p1_prolongate_cell(coarse.data_ptr(), fine.data_ptr(), lc, ones, capi.REPLACE)
    torch.cuda.synchronize()
    assert float(fine.min()) == 1.0 and float(fine.max()) == 1.0
    coarse = linear(lc)
    assert coarse.numel() == nc
    capi.p1_prolongate_cell(coarse.data_ptr(), fine.data_ptr(), lc, ones, capi.REPLACE)
    torch.cuda.synchronize()
    want = linear(lf)
    assert float((fine - want).abs().max()) <= 1e-13 * float(want.abs().max())
    del want
    fine.fill_(1.0)
    capi.p1_restrict_cell(coarse.data_ptr(), fine.data_ptr(), lc, ones)
    torch.cuda.synchronize()
    assert float(coarse[capi.cell_index(lc, 3, 4, 5)]) == 8.0 and float(coarse.max()) == 8.0
