"""GPU tests of the batched kernels (one launch for all macro-cells of a rank, inner and boundary points together):
the C-ABI entry points against the CPU oracle applied cell by cell, and the host layer with batching on against the same
host layer with batching off (per-cell kernels) on whole V-cycles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _cells(po, level):
    """three cells of regular_octahedron_8el with their stencil tables [15][15] (rows 0..13 shares, 14 inner)"""
    import hostutil as hu

    v, c = hu.read_msh(hu.MESHES / "regular_octahedron_8el.msh")
    tabs = []
    for cv in c[[0, 3, 6]]:
        co = v[cv].reshape(12)
        tabs.append(np.vstack([po.assemble_cell_slot_stencils(co, level).reshape(14, 15), po.assemble_cell_stencil(co, level)[None, :]]))
    return np.array(tabs)


MASKS = [0x7FFF, 0x4000 | 0x2A5, 0x3FFF]


def _oracle_apply(po, dst, src, level, tab, mask, update):
    if (mask & po.MASK_INNER) and level >= 2:
        po.apply_cell(dst, src, level, tab[14], update)
    po.apply_cell_boundary(dst, src, level, tab[:14].reshape(-1), mask & po.MASK_SHELL, update)
    return dst


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("update", [0, 1])
def test_apply_cells_matches_the_oracle_cell_by_cell(env, level, update):
    torch, capi, host, po = env
    tabs = _cells(po, level)
    n = po.cell_size(level)
    rng = np.random.default_rng(level)
    src = [rng.standard_normal(n) for _ in range(3)]
    dst0 = [rng.standard_normal(n) for _ in range(3)]
    dsrc, ddst, dtab = [_dev(torch, a) for a in src], [_dev(torch, a) for a in dst0], _dev(torch, tabs.reshape(-1))
    capi.p1_apply_cells([t.data_ptr() for t in ddst], [t.data_ptr() for t in dsrc], level, dtab.data_ptr(), MASKS, update)
    torch.cuda.synchronize()
    for c in range(3):
        want = _oracle_apply(po, dst0[c].copy(), src[c], level, tabs[c], MASKS[c], update)
        got = ddst[c].cpu().numpy()
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("level", [0, 2, 4])
def test_vector_and_dot_cells(env, level):
    torch, capi, host, po = env
    import hostutil as hu

    n = po.cell_size(level)
    rng = np.random.default_rng(10 + level)
    a, b, d0 = ([rng.standard_normal(n) for _ in range(3)] for _ in range(3))
    for op, scalars in ((0, [2.0, -0.5]), (1, [0.25, 3.0]), (2, None), (3, [7.5])):
        da, db, dd = [_dev(torch, x) for x in a], [_dev(torch, x) for x in b], [_dev(torch, x) for x in d0]
        srcs = [] if op == 3 else [[t.data_ptr() for t in da], [t.data_ptr() for t in db]]
        capi.p1_vector_cells(op, [t.data_ptr() for t in dd], srcs, scalars, level, MASKS)
        torch.cuda.synchronize()
        for c in range(3):
            sel = hu.point_mask(level, MASKS[c])
            if op == 0:
                want = 2.0 * a[c] - 0.5 * b[c]
            elif op == 1:
                want = d0[c] + (0.25 * a[c] + 3.0 * b[c])
            elif op == 2:
                want = a[c] * b[c]
            else:
                want = np.full(n, 7.5)
            got = dd[c].cpu().numpy()
            assert np.array_equal(got[~sel], d0[c][~sel])
            assert np.abs(got[sel] - want[sel]).max() <= 1e-14 * max(1.0, np.abs(want).max()) if sel.any() else True
    da, db = [_dev(torch, x) for x in a], [_dev(torch, x) for x in b]
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    capi.p1_dot_cells([t.data_ptr() for t in da], [t.data_ptr() for t in db], level, MASKS, res.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    want = sum(po.dot_cell_masked(a[c], b[c], level, MASKS[c]) for c in range(3))
    assert abs(float(res[0]) - want) <= 1e-13 * max(1.0, abs(want))


@pytest.mark.parametrize("coarse_level", [0, 1, 3])
def test_grid_transfer_cells_match_the_per_cell_kernels(env, coarse_level):
    """same terms and order as the per-cell masked kernels: bit-identical"""
    torch, capi, host, po = env
    nc, nf = po.cell_size(coarse_level), po.cell_size(coarse_level + 1)
    rng = np.random.default_rng(coarse_level)
    nnc = np.array([[1, 2, 4, 1, 3, 2, 1, 2, 2, 1, 5, 4, 3, 8], [2] * 14, [1] * 14], dtype=np.float64)
    dinv = _dev(torch, (1.0 / nnc).reshape(-1))
    fine, coarse = [rng.standard_normal(nf) for _ in range(3)], [rng.standard_normal(nc) for _ in range(3)]
    # restriction
    df, dc, dc2 = [_dev(torch, x) for x in fine], [_dev(torch, x) for x in coarse], [_dev(torch, x) for x in coarse]
    capi.p1_restrict_cells([t.data_ptr() for t in dc], [t.data_ptr() for t in df], coarse_level, dinv.data_ptr(), MASKS)
    for c in range(3):
        capi.p1_restrict_cell_masked(dc2[c].data_ptr(), df[c].data_ptr(), coarse_level, nnc[c], MASKS[c])
    torch.cuda.synchronize()
    for c in range(3):
        assert np.array_equal(dc[c].cpu().numpy(), dc2[c].cpu().numpy())
    # prolongation (Replace on the masked points)
    dc = [_dev(torch, x) for x in coarse]
    df, df2 = [_dev(torch, x) for x in fine], [_dev(torch, x) for x in fine]
    capi.p1_prolongate_cells([t.data_ptr() for t in dc], [t.data_ptr() for t in df], coarse_level, dinv.data_ptr(), MASKS)
    for c in range(3):
        capi.p1_prolongate_cell_masked(dc[c].data_ptr(), df2[c].data_ptr(), coarse_level, nnc[c], MASKS[c])
    torch.cuda.synchronize()
    for c in range(3):
        assert np.array_equal(df[c].cpu().numpy(), df2[c].cpu().numpy())


def test_batched_calls_reject_bad_arguments(env):
    torch, capi, host, po = env
    a = _dev(torch, np.zeros(po.cell_size(2)))
    with pytest.raises(capi.HytegHipError):
        capi.p1_vector_cells(0, [a.data_ptr()] * 81, [[a.data_ptr()] * 81], [1.0], 2, [0x7FFF] * 81)  # > HYTEG_HIP_MAX_BATCH
    with pytest.raises(capi.HytegHipError):
        capi.p1_apply_cells([a.data_ptr()], [a.data_ptr()], 2, a.data_ptr(), [0x7FFF])  # dst aliases src


def _vcycle(host, mesh, lo, hi, smoother, batch):
    import hostutil as hu

    st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
    st.set_batch_max_level(batch)
    mo = hu.MultiCellOracle(st)
    A = host.P1ConstantOperator(st, lo, hi)
    A.compute_inverse_diagonal()
    x, b, r = (host.P1Function(st, n, lo, hi) for n in ("x", "b", "r"))
    hu.upload(x, mo.interpolate(lambda X, Y, Z: np.sin(11 * X) * np.cos(5 * Y) + Z * X, hi), hi)
    x.interpolate(0.0, hi, host.DirichletBoundary)
    hu.upload(b, mo.interpolate(lambda X, Y, Z: 1.0 + X - Y * Z, hi), hi)
    gmg = host.Solver.gmg(st, lo, hi, smoother=smoother, relax=2.0 / 3.0, pre=2, post=2, cg_max_iter=30, cg_tol=1e-12)
    gmg.solve(A, x, b, hi)
    A.apply(x, r, hi, host.Inner)
    out = hu.download(x, hi), hu.download(r, hi), r.dot(r, hi, host.Inner)
    for o in (gmg, x, b, r, A, st):
        o.close()
    return out


@pytest.mark.parametrize("mesh,lo,hi,smoother", [("regular_octahedron_8el", 0, 4, "GAUSS_SEIDEL"), ("regular_octahedron_8el", 2, 4, "JACOBI"),
                                                  ("cube_6el", 1, 3, "JACOBI"), ("pyramid_tilted_4el", 0, 3, "GAUSS_SEIDEL")])
def test_vcycle_with_batched_kernels_equals_the_per_cell_kernels(env, mesh, lo, hi, smoother):
    torch, capi, host, po = env
    xb, rb, db = _vcycle(host, mesh, lo, hi, getattr(host, smoother), 6)
    xc, rc, dc = _vcycle(host, mesh, lo, hi, getattr(host, smoother), -1)
    scale = max(np.abs(a).max() for a in xc)
    for a, b in zip(xb, xc):
        assert np.abs(a - b).max() <= 1e-11 * scale
    assert abs(db - dc) <= 1e-9 * abs(dc)


def test_gauss_seidel_sweeps_shared_between_cells_above_the_batch_level(env):
    """Above the batch level only the Gauss-Seidel / SOR sweeps (macro-cell sweep, rest, shell sweeps) share their launches
    between the cells of a rank (PrimitiveStorage::useBatchSor): a V(2,2) cycle over levels 6-7 of a 2-cell mesh with the batch
    level at 5 against the same cycle with per-cell launches throughout."""
    torch, capi, host, po = env
    xb, rb, db = _vcycle(host, "pyramid_2el", 6, 7, host.GAUSS_SEIDEL, 5)
    xc, rc, dc = _vcycle(host, "pyramid_2el", 6, 7, host.GAUSS_SEIDEL, -1)
    scale = max(np.abs(a).max() for a in xc)
    for a, b in zip(xb, xc):
        assert np.abs(a - b).max() <= 1e-11 * scale
    assert abs(db - dc) <= 1e-9 * abs(dc)


@pytest.mark.parametrize("level", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("backwards", [False, True])
def test_sor_cells_match_the_per_cell_sweeps(env, level, backwards):
    """levels <= 4: same update and summation order as the per-cell plane kernel (bit-identical); level 5 is compared
    with the blocked per-cell kernel (other summation order inside an update), level 6 is the same blocked kernel batched"""
    torch, capi, host, po = env
    tabs = _cells(po, level)
    n = po.cell_size(level)
    rng = np.random.default_rng(level)
    u0, b = [rng.standard_normal(n) for _ in range(3)], [rng.standard_normal(n) for _ in range(3)]
    masks = [0x7FFF, 0x3FFF, 0x4000]  # the middle cell has no inner points selected: untouched
    du, db, dtab = [_dev(torch, a) for a in u0], [_dev(torch, a) for a in b], _dev(torch, tabs.reshape(-1))
    capi.p1_sor_cells([t.data_ptr() for t in du], [t.data_ptr() for t in db], level, dtab.data_ptr(), 1.15, masks, backwards)
    torch.cuda.synchronize()
    for c in range(3):
        got = du[c].cpu().numpy()
        if not masks[c] & po.MASK_INNER:
            assert np.array_equal(got, u0[c])
            continue
        ref = _dev(torch, u0[c])
        capi.p1_sor_cell(ref.data_ptr(), db[c].data_ptr(), level, list(tabs[c][14]), 1.15, backwards)
        torch.cuda.synchronize()
        want = ref.cpu().numpy()
        if level == 5:
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        else:
            assert np.array_equal(got, want)
        oracle = po.sor_cell(u0[c].copy(), b[c], level, tabs[c][14], 1.15, backwards)
        assert np.abs(got - oracle).max() <= 1e-12 * np.abs(oracle).max()


@pytest.mark.parametrize("level", [0, 1, 2, 4, 6])
@pytest.mark.parametrize("backwards", [False, True])
def test_sor_shell_cells_match_the_per_cell_kernel(env, level, backwards):
    torch, capi, host, po = env
    import hostutil as hu

    v, c = hu.read_msh(hu.MESHES / "regular_octahedron_8el.msh")
    tables = [hu.sor_tables(v, c, level)[k] for k in (1, 4, 7)]
    n = po.cell_size(level)
    rng = np.random.default_rng(40 + level)
    u0, b, rest = ([rng.standard_normal(n) for _ in range(3)] for _ in range(3))
    masks = [0x3FFF, 0x2A5 | (0x5 << 10), 0x3C0]
    raw = np.frombuffer(capi.sor_shell_tables_bytes(tables), dtype=np.uint8).copy()
    dtab = torch.from_numpy(raw).to("cuda")
    du, db, dr = ([_dev(torch, a) for a in arrs] for arrs in (u0, b, rest))
    capi.p1_sor_shell_cells([t.data_ptr() for t in du], [t.data_ptr() for t in db], [t.data_ptr() for t in dr], level, dtab.data_ptr(), 1.1,
                            masks, backwards)
    torch.cuda.synchronize()
    for k, t in enumerate(tables):
        ref, rr = _dev(torch, u0[k]), _dev(torch, rest[k])
        capi.p1_sor_shell_cell(ref.data_ptr(), db[k].data_ptr(), rr.data_ptr(), level, t["edge_verts"], t["edge_w"], t["face_verts"],
                               t["face_w"], t["vertex_w"], 1.1, masks[k], backwards)
        torch.cuda.synchronize()
        assert np.array_equal(du[k].cpu().numpy(), ref.cpu().numpy())


# ---- the batched entry points one by one, against the oracle and numpy ---------------------------------------------------
def _oracle_share(po, src, level, tab):
    """(A src on the inner points, the cell's share of A src on the shell points) in one array, zero where neither writes"""
    out = np.zeros_like(src)
    if level >= 2:
        po.apply_cell(out, src, level, tab[14], po.REPLACE)
    po.apply_cell_boundary(out, src, level, tab[:14].reshape(-1), po.MASK_SHELL, po.REPLACE)
    return out


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("phase", [0, 1])
def test_jacobi_cells_phases_match_the_oracle(env, level, phase):
    """phase 0: the complete update on selected inner points, the cell's share of A src on selected shell points;
    phase 1: dst = src + relax * invdiag * (rhs - dst) on selected shell points, inner points untouched (bit 14 or not);
    every mask of MASKS and a zero mask visits every cell"""
    torch, capi, host, po = env
    import hostutil as hu

    tabs = _cells(po, level)
    n = po.cell_size(level)
    rng = np.random.default_rng(50 + level)
    src, rhs, dst0 = ([rng.standard_normal(n) for _ in range(3)] for _ in range(3))
    invd = [rng.uniform(0.5, 1.5, n) for _ in range(3)]
    relax = 0.7
    assert all(np.abs(r).min() > 0 for r in rhs)
    dsrc, drhs, dinv = ([_dev(torch, a) for a in arrs] for arrs in (src, rhs, invd))
    dtab = _dev(torch, tabs.reshape(-1))
    inner = po.slot_of_points(level) == 14
    assert inner.any() == (level >= 2)
    all_masks = MASKS + [0]
    checked = 0
    for rot in range(len(all_masks)):
        masks = [all_masks[(rot + c) % len(all_masks)] for c in range(3)]
        ddst = [_dev(torch, a) for a in dst0]
        capi.p1_jacobi_cells([t.data_ptr() for t in ddst], [t.data_ptr() for t in drhs], [t.data_ptr() for t in dsrc], [t.data_ptr() for t in dinv],
                             level, dtab.data_ptr(), relax, masks, phase)
        for c in range(3):
            got = ddst[c].cpu().numpy()
            sel = hu.point_mask(level, masks[c])
            assert np.array_equal(got[~sel], dst0[c][~sel])
            if phase == 0:
                asrc = _oracle_share(po, src[c], level, tabs[c])
                want = np.where(inner, src[c] + relax * invd[c] * (rhs[c] - asrc), asrc)
                cmp = sel
            else:
                want = src[c] + relax * (invd[c] * (rhs[c] - dst0[c]))
                cmp = sel & ~inner
                assert np.array_equal(got[inner], dst0[c][inner])
            if masks[c] == 0:
                assert np.array_equal(got, dst0[c])
            if cmp.any():
                assert np.abs(got[cmp] - want[cmp]).max() <= 1e-13 * max(1.0, np.abs(want).max()), (hex(masks[c]), c)
                checked += int(cmp.sum())
    assert checked > 0


@pytest.mark.parametrize("level", [0, 2, 4])
@pytest.mark.parametrize("nsrc", [1, 3, 4])
def test_vector_cells_with_one_three_and_four_sources(env, level, nsrc):
    """batch_vector_kernel<1>, <3> and <4> against numpy (the two-source instantiation is test_vector_and_dot_cells)"""
    torch, capi, host, po = env
    import hostutil as hu

    n = po.cell_size(level)
    rng = np.random.default_rng(60 + 10 * level + nsrc)
    srcs = [[rng.standard_normal(n) for _ in range(3)] for _ in range(nsrc)]
    d0 = [rng.standard_normal(n) for _ in range(3)]
    scalars = [2.0, -0.5, 0.25, 3.0][:nsrc]
    dsrc = [[_dev(torch, a) for a in f] for f in srcs]
    checked = 0
    for op in (0, 1, 2):
        dd = [_dev(torch, x) for x in d0]
        capi.p1_vector_cells(op, [t.data_ptr() for t in dd], [[t.data_ptr() for t in f] for f in dsrc], None if op == 2 else scalars, level, MASKS)
        for c in range(3):
            sel = hu.point_mask(level, MASKS[c])
            if op == 2:
                want = srcs[0][c].copy()
                for k in range(1, nsrc):
                    want = want * srcs[k][c]
            else:
                want = scalars[0] * srcs[0][c]
                for k in range(1, nsrc):
                    want = want + scalars[k] * srcs[k][c]
                if op == 1:
                    want = d0[c] + want
            got = dd[c].cpu().numpy()
            assert np.array_equal(got[~sel], d0[c][~sel])
            if sel.any():
                assert np.abs(got[sel] - want[sel]).max() <= 1e-14 * max(1.0, np.abs(want).max())
                checked += 1
            else:  # level 0 is four macro-vertices, and the mask of cell 1 has no vertex slot
                assert level == 0 and c == 1 and not MASKS[c] & 0x3C00
    assert checked == (6 if level == 0 else 9)


def _full_tiles_per_cell(level, capacity=256):
    """workgroups per cell of the batched kernels: every z-slice of the array in balanced tiles of at most `capacity` entries"""
    N = (1 << level) + 1
    return sum(((N - z) * (N - z + 1) // 2 + capacity - 1) // capacity for z in range(N))


@pytest.mark.parametrize("ncells,level,regime", [(3, 2, "one launch"), (3, 5, "two launches"), (5, 6, "grid stride")])
def test_dot_cells_in_its_three_launch_regimes(env, ncells, level, regime):
    """up to 64 workgroups: the last one to finish reduces; 65..1023: a second launch reduces; from 1024 tiles on, 1024 workgroups
    walk several tiles each.  Twice on the same workspace: the ticket counter of the first regime has to be back at zero for
    the second call to write a result at all, and the fixed summation order makes the two results bit-identical."""
    import math

    torch, capi, host, po = env
    import hostutil as hu

    total = ncells * _full_tiles_per_cell(level)
    assert {"one launch": total <= 64, "two launches": 64 < total < 1024, "grid stride": total > 1024}[regime], total
    n = po.cell_size(level)
    rng = np.random.default_rng(70 + level)
    a, b = rng.standard_normal((ncells, n)), rng.standard_normal((ncells, n))
    masks = [(MASKS + [1 << 14, 0x4000 | 0x03C0])[c % 5] for c in range(ncells)]
    ta, tb = _dev(torch, a), _dev(torch, b)
    prods = np.concatenate([(a[c] * b[c])[hu.point_mask(level, masks[c])] for c in range(ncells)])
    ref, scale = math.fsum(prods), float(np.abs(prods).sum())
    ws = torch.full((capi.dot_workspace_bytes() // 8,), 1e300, dtype=torch.float64, device="cuda")
    got = []
    for _ in range(2):
        res = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
        capi.p1_dot_cells([ta[c].data_ptr() for c in range(ncells)], [tb[c].data_ptr() for c in range(ncells)], level, masks, res.data_ptr(),
                          ws.data_ptr())
        got.append(float(res.cpu()[0]))
        assert abs(got[-1] - ref) <= 1e-13 * scale, (got, ref, scale)
    assert got[0] == got[1] and len(prods) > 0


@pytest.mark.parametrize("coarse_level", [0, 2, 3, 4])
@pytest.mark.parametrize("update", [0, 1])
def test_prolongate_cell_masked_update(env, coarse_level, update):
    """fine level 1 and 3: the tile kernel, 4 and 5: the brick kernel.  ADD adds the interpolant to the selected inner points
    and overwrites the selected shell points; REPLACE overwrites the selected points; everything else keeps its bits."""
    torch, capi, host, po = env
    import hostutil as hu

    nnc = [3, 4, 5, 6, 7, 8, 2, 1, 2, 2, 9, 10, 11, 12]  # _NNC_MIXED of test_gpu_parity.py
    fl = coarse_level + 1
    rng = np.random.default_rng(80 + coarse_level)
    coarse_h, fine0 = rng.standard_normal(po.cell_size(coarse_level)), rng.standard_normal(po.cell_size(fl))
    full = po.prolongate_cell(coarse_h, np.zeros_like(fine0), coarse_level, np.array(nnc, dtype=np.float64))
    inner = po.slot_of_points(fl) == 14
    coarse = _dev(torch, coarse_h)
    checked = 0
    for mask in (0x7FFF, 1 << 14, 0x4000 | 0x03C0, 0x3FFF):
        fine = _dev(torch, fine0)
        capi.p1_prolongate_cell_masked_update(coarse.data_ptr(), fine.data_ptr(), coarse_level, nnc, mask, update)
        got = fine.cpu().numpy()
        sel = hu.point_mask(fl, mask)
        want = np.where(sel, np.where(inner & (update == capi.ADD), fine0 + full, full), fine0)
        assert np.array_equal(got[~sel], fine0[~sel]), hex(mask)
        nw = np.linalg.norm(want)
        assert np.linalg.norm(got - want) / (nw if nw > 0 else 1.0) < 1e-13, hex(mask)  # TOL and _rel of test_gpu_host.py
        if sel.any():
            assert np.abs(got[sel] - want[sel]).max() <= 1e-13 * np.abs(want).max(), hex(mask)
        checked += int(sel.sum())
    assert checked > 0


@pytest.mark.parametrize("level", [0, 1, 3, 5])
@pytest.mark.parametrize("tet", ["REF_TET", "SKEW_TET"])
def test_apply_cell_boundary_f32_matches_the_oracle_in_double(env, level, tet):
    """the float instantiation on its own: REPLACE and ADD, against the double oracle on float32-representable inputs"""
    torch, capi, host, po = env
    import conftest
    import hostutil as hu

    ws = po.assemble_cell_slot_stencils(getattr(conftest, tet), level)
    n = po.cell_size(level)
    rng = np.random.default_rng(90 + level)
    src32, d32 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    src64, d64 = src32.astype(np.float64), d32.astype(np.float64)
    dsrc = _dev(torch, src32)
    checked = 0
    for mask in (0x3FFF, 0x2A5, 0):
        sel = hu.point_mask(level, mask)
        for update in (capi.REPLACE, capi.ADD):
            dst = _dev(torch, d32)
            capi.p1_apply_cell_boundary_f32(dst.data_ptr(), dsrc.data_ptr(), level, ws, mask, update)
            got = dst.cpu().numpy()
            assert got.dtype == np.float32
            assert np.array_equal(got[~sel], d32[~sel])
            want = po.apply_cell_boundary(d64.copy(), src64, level, ws, mask, update)
            if sel.any():
                assert np.linalg.norm(got[sel] - want[sel]) / np.linalg.norm(want[sel]) < 2e-6  # F32_TOL of test_gpu_fp32.py
                checked += int(sel.sum())
            else:  # the zero mask, and at level 0 (four vertices) the mask without a vertex slot
                assert mask == 0 or (level == 0 and not mask & 0x3C00)
                assert np.array_equal(got, d32)
    assert checked > 0
