"""GPU tests of the edge-DoF vector operations and dot products (hyteg_amd/csrc/p2_edge_vector.hip) entry by entry: the
C-ABI calls against numpy on the oracle's own indexing (po.edge_coords: x, y, z, orientation of every array entry;
po.edge_classes: its point class).  An entry takes part when (mask >> class) & 1 and (kind_mask >> (orientation + 1)) & 1."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASKS = [0x7FFF, 0x4000 | 0x2A5, 0x3FFF, 1 << 14, 0]
KINDS = [0xFE] + [1 << k for k in range(1, 8)] + [0x54]
SCALARS = [2.0, -0.5, 0.25, 3.0]
SENTINEL = 1e300


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi, po


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _selected(po, level, mask, kinds=0xFE):
    """boolean per edge-array entry, from the oracle's classes and orientations"""
    cls, o = po.edge_classes(level), po.edge_coords(level)[:, 3]
    return (((mask >> cls) & 1) & ((kinds >> (o + 1)) & 1)).astype(bool)


def _want(op, d0, srcs, scalars):
    """the kernel's expression, term by term in its order"""
    if op == 3:
        return np.full_like(d0, scalars[0])
    if op == 2:
        tmp = srcs[0].copy()
        for s in srcs[1:]:
            tmp = tmp * s
        return tmp
    tmp = scalars[0] * srcs[0]
    for c, s in zip(scalars[1:], srcs[1:]):
        tmp = tmp + c * s
    return d0 + tmp if op == 1 else tmp


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_vector_cell_kinds_matches_numpy_entry_by_entry(env, level, op):
    """every (sources, point mask, kind mask): selected entries against numpy at the batched vector test's tolerance,
    every other entry bit-identical to what was there; _cell_masked has the bits of _cell_kinds(..., 0xFE)"""
    torch, capi, po = env
    n = po.edge_array_size(level)
    assert n == capi.p2_edge_array_size(level) == len(po.edge_classes(level)) and n == {0: 6, 1: 25}.get(level, n)
    rng = np.random.default_rng(100 + level)
    src_h, d0 = [rng.standard_normal(n) for _ in range(4)], rng.standard_normal(n)
    src_d, d0_d = [_dev(torch, a) for a in src_h], _dev(torch, d0)
    checked = 0
    for nsrc in (1, 2, 4):
        srcs, sc = src_h[:nsrc], SCALARS[:nsrc]
        want = _want(op, d0, srcs, sc)
        ptrs = [t.data_ptr() for t in src_d[:nsrc]]
        for mask in MASKS:
            for kinds in KINDS:
                sel = _selected(po, level, mask, kinds)
                dst = d0_d.clone()
                capi.p2_edge_vector_cell_kinds(op, dst.data_ptr(), ptrs, None if op == 2 else sc, level, mask, kinds)
                got = dst.cpu().numpy()
                assert np.array_equal(got[~sel], d0[~sel]), (nsrc, hex(mask), hex(kinds))
                if sel.any():
                    assert np.abs(got[sel] - want[sel]).max() <= 1e-14 * max(1.0, np.abs(want).max()), (nsrc, hex(mask), hex(kinds))
                    checked += int(sel.sum())
                if kinds == 0xFE:
                    dst2 = d0_d.clone()
                    capi.p2_edge_vector_cell_masked(op, dst2.data_ptr(), ptrs, None if op == 2 else sc, level, mask)
                    assert np.array_equal(dst2.cpu().numpy(), got)
    assert checked > 0
    # the full mask with every orientation writes every entry, whatever the level
    assert _selected(po, level, 0x7FFF).all()


def test_vector_cell_zero_mask_changes_nothing(env):
    torch, capi, po = env
    level = 3
    n = po.edge_array_size(level)
    rng = np.random.default_rng(7)
    a, d0 = rng.standard_normal(n), rng.standard_normal(n)
    da = _dev(torch, a)
    for op in range(4):
        for mask, kinds in ((0, 0xFE), (0x7FFF, 0), (0x7FFF, 0x01), (0x8000, 0xFE)):
            dst = _dev(torch, d0)
            capi.p2_edge_vector_cell_kinds(op, dst.data_ptr(), [da.data_ptr()], [1.5], level, mask, kinds)
            assert np.array_equal(dst.cpu().numpy(), d0)


def _batch_masks(ncells):
    """a different mask per cell; cell 1 (cell 0 of a single-cell batch excepted) has mask 0"""
    base = [0x4000 | 0x2A5, 0, 0x3FFF, 1 << 14, 0x7FFF]
    more = [int(m) for m in np.random.default_rng(ncells).permutation(np.arange(1, 0x7FFF)) if int(m) not in base]
    return (base + more)[:ncells]


@pytest.mark.parametrize("ncells,level", [(1, 2), (3, 2), (80, 2), (3, 4)])
def test_vector_cells_kinds_has_the_bits_of_the_per_cell_call(env, ncells, level):
    """same expression in the same order, one launch for the batch"""
    torch, capi, po = env
    assert ncells <= capi.HYTEG_HIP_MAX_BATCH
    n = po.edge_array_size(level)
    rng = np.random.default_rng(level * 100 + ncells)
    src = rng.standard_normal((4, ncells, n))
    d0 = rng.standard_normal((ncells, n))
    src_d, d0_d = _dev(torch, src), _dev(torch, d0)  # row [k, c] / [c] is the array of one cell
    masks = _batch_masks(ncells)
    assert len(set(masks)) == ncells and (ncells == 1 or masks[1] == 0)
    changed = 0
    for op in range(4):
        for nsrc in (1, 3, 4):
            for kinds in (0xFE, 0x54):
                sc = None if op == 2 else SCALARS[:nsrc]
                batch, single = d0_d.clone(), d0_d.clone()
                capi.p2_edge_vector_cells_kinds(op, [batch[c].data_ptr() for c in range(ncells)],
                                                [[src_d[k, c].data_ptr() for c in range(ncells)] for k in range(nsrc)], sc, level, masks, kinds)
                for c in range(ncells):
                    capi.p2_edge_vector_cell_kinds(op, single[c].data_ptr(), [src_d[k, c].data_ptr() for k in range(nsrc)], sc, level, masks[c],
                                                   kinds)
                batch_h, single_h = batch.cpu().numpy(), single.cpu().numpy()
                for c in range(ncells):
                    got = batch_h[c]
                    assert np.array_equal(got, single_h[c]), (op, nsrc, hex(kinds), c)
                    sel = _selected(po, level, masks[c], kinds)
                    assert np.array_equal(got[~sel], d0[c][~sel])
                    if sel.any():
                        assert not np.array_equal(got[sel], d0[c][sel])
                        changed += 1
    assert changed > 0


def _dot_ref(po, a, b, level, mask):
    sel = _selected(po, level, mask)
    prod = (a * b)[sel]
    return math.fsum(prod), float(np.abs(prod).sum()), int(sel.sum())


@pytest.mark.parametrize("level", [0, 1, 3, 5, 6])
def test_edge_dot_cell_masked_against_an_exact_sum(env, level):
    """level 6 has 318 240 entries > 1024 x 256: the smallest level at which a workgroup of p2_edge_dot_kernel strides"""
    torch, capi, po = env
    n = po.edge_array_size(level)
    assert (n > 1024 * 256) == (level == 6)
    rng = np.random.default_rng(200 + level)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    da, db = _dev(torch, a), _dev(torch, b)
    counted = 0
    for mask in MASKS:
        res = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
        ws = torch.full((capi.dot_workspace_bytes() // 8,), SENTINEL, dtype=torch.float64, device="cuda")
        capi.p2_edge_dot_cell_masked(da.data_ptr(), db.data_ptr(), level, mask, res.data_ptr(), ws.data_ptr())
        got = float(res.cpu()[0])
        ref, scale, count = _dot_ref(po, a, b, level, mask)
        if mask == 0:
            assert count == 0 and got == 0.0
        assert abs(got - ref) <= 1e-13 * scale, (hex(mask), got, ref, scale)
        counted += count
    assert counted > 0


@pytest.mark.parametrize("ncells,level", [(3, 2), (80, 2), (3, 5)])
def test_edge_dot_cells_masked_per_cell_results(env, ncells, level):
    torch, capi, po = env
    n = po.edge_array_size(level)
    rng = np.random.default_rng(300 + level + ncells)
    a, b = rng.standard_normal((ncells, n)), rng.standard_normal((ncells, n))
    ta, tb = _dev(torch, a), _dev(torch, b)
    da, db = [ta[c] for c in range(ncells)], [tb[c] for c in range(ncells)]
    masks = _batch_masks(ncells)
    res = torch.full((ncells + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    capi.p2_edge_dot_cells_masked([t.data_ptr() for t in da], [t.data_ptr() for t in db], level, masks, res.data_ptr())
    got = res.cpu().numpy()
    assert got[ncells] == SENTINEL  # nothing is written past the last cell
    counted = 0
    for c in range(ncells):
        ref, scale, count = _dot_ref(po, a[c], b[c], level, masks[c])
        if masks[c] == 0:
            assert count == 0 and got[c] == 0.0
        assert abs(got[c] - ref) <= 1e-13 * scale, (c, hex(masks[c]), got[c], ref, scale)
        counted += count
    assert masks[1] == 0 and counted > 0


def test_edge_calls_reject_bad_arguments(env):
    torch, capi, po = env
    a = _dev(torch, np.zeros(po.edge_array_size(2)))
    p = a.data_ptr()
    res = torch.zeros(81, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.HytegHipError):  # ncells = HYTEG_HIP_MAX_BATCH + 1
        capi.p2_edge_vector_cells_kinds(0, [p] * 81, [[p] * 81], [1.0], 2, [0x7FFF] * 81)
    with pytest.raises(capi.HytegHipError):
        capi.p2_edge_dot_cells_masked([p] * 81, [p] * 81, 2, [0x7FFF] * 81, res.data_ptr())
    for level in (10, -1):  # HYTEG_HIP_P2_MAX_LEVEL is 9
        with pytest.raises(capi.HytegHipError):
            capi.p2_edge_vector_cell_kinds(0, p, [p], [1.0], level, 0x7FFF, 0xFE)
        with pytest.raises(capi.HytegHipError):
            capi.p2_edge_vector_cell_masked(0, p, [p], [1.0], level, 0x7FFF)
        with pytest.raises(capi.HytegHipError):
            capi.p2_edge_vector_cells_kinds(0, [p], [[p]], [1.0], level, [0x7FFF])
        with pytest.raises(capi.HytegHipError):
            capi.p2_edge_dot_cell_masked(p, p, level, 0x7FFF, res.data_ptr(), res.data_ptr())
        with pytest.raises(capi.HytegHipError):
            capi.p2_edge_dot_cells_masked([p], [p], level, [0x7FFF], res.data_ptr())
    with pytest.raises(capi.HytegHipError):  # op = 4
        capi.p2_edge_vector_cell_kinds(4, p, [p], [1.0], 2, 0x7FFF, 0xFE)
    with pytest.raises(capi.HytegHipError):
        capi.p2_edge_vector_cells_kinds(4, [p], [[p]], [1.0], 2, [0x7FFF])
    with pytest.raises(capi.HytegHipError):  # five sources
        capi.p2_edge_vector_cell_kinds(0, p, [p] * 5, [1.0] * 5, 2, 0x7FFF, 0xFE)
    with pytest.raises(capi.HytegHipError):
        capi.p2_edge_vector_cells_kinds(0, [p], [[p]] * 5, [1.0] * 5, 2, [0x7FFF])
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), np.zeros(po.edge_array_size(2)))
