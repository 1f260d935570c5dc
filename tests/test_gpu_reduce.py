"""GPU tests of the statistics reduction (hyteg_hip_p1_reduce_cells in hyteg_amd/csrc/p1_batch.hip,
hyteg_hip_p2_edge_reduce_cells in p2_edge_vector.hip) entry by entry through the C-ABI: sum, sum of magnitudes, min, max
and max magnitude of the selected entries of every cell against numpy / math.fsum on the oracle's own indexing
(hostutil.point_mask, po.edge_classes).

Workgroups per cell: a cell's array is cut into tiles of 256 entries; up to 32 tiles ONE workgroup walks the cell, above that
min(tiles, 1024) workgroups do and a second launch folds their partial results.  The vertex-DoF array has 17 tiles at level 4
and 46 at level 5 (tiles do not cross z-slices), the edge-DoF array 22 at level 4 and 162 at level 5: for both forms level 5 is
the smallest level with more than one workgroup per cell, and it is tested.  Level 8 (vertex form, 11,400 tiles) and level 6
(edge form, 318,240 entries = 1,244 tiles) are the smallest levels at which a workgroup takes more than one tile (1024 workgroups
per cell).

Unselected entries hold +-1e300, so an entry that leaks into the reduction shows in all five numbers.  Min, max and max magnitude
must equal numpy's exactly.  The sums must satisfy |got - fsum| <= 1e-12 * sum|x|, the project's fp64 parity bound: every
summation order errs by a small multiple of eps * sum|x| (here at most ~60 additions deep: 7e-15), while one dropped or doubled
standard normal is O(0.1 - 1) against a bound of about 2e-6 at level 8."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASKS = [0x7FFF, 0x4000 | 0x2A5, 0x3FFF, 1 << 14, 0, 1 << 3, 1 << 7, 1 << 12]
SENTINEL = 1e300
DBL_MAX = float(np.finfo(np.float64).max)
EMPTY = [0.0, 0.0, DBL_MAX, -DBL_MAX, 0.0]
MAX_BATCH = 80


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    assert capi.HYTEG_HIP_MAX_BATCH == MAX_BATCH and capi.REDUCE_COUNT == 5
    ws = torch.empty(capi.reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    return torch, capi, po, ws


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _slots(po, level):
    """po.slot_of_points(level) without a Python loop per point (level 8 has 2.9 million): the same face flags on po.cell_coords"""
    c, n = po.cell_coords(level), po.width(level)
    f = [c[:, 2] == 0, c[:, 1] == 0, c[:, 0] == 0, c.sum(axis=1) == n - 1]
    key = f[0] * 1 + f[1] * 2 + f[2] * 4 + f[3] * 8
    table = np.full(16, -1)
    table[0] = 14
    table[[1, 2, 4, 8]] = [6, 7, 8, 9]
    table[[3, 5, 9, 6, 10, 12]] = [0, 1, 2, 3, 4, 5]
    table[[7, 11, 13, 14]] = [10, 11, 12, 13]
    out = table[key]
    assert (out >= 0).all()
    return out


def _vertex_selected(po, level, mask):
    import hostutil

    if level <= 6:
        return hostutil.point_mask(level, mask)
    return ((mask >> _slots(po, level)) & 1).astype(bool)


def _edge_selected(po, level, mask):
    """the `_selected` of test_gpu_p2_edge_vector.py with every orientation"""
    return ((mask >> po.edge_classes(level)) & 1).astype(bool)


def _field(seed, sel):
    """standard normals on the selected entries, +-1e300 everywhere else"""
    x = np.random.default_rng(seed).standard_normal(sel.size)
    return np.where(sel, x, np.where(np.arange(sel.size) % 2 == 0, SENTINEL, -SENTINEL))


def _check(got, x, tag):
    got = [float(v) for v in got]
    if x.size == 0:
        assert got == EMPTY, tag
        return
    sabs = math.fsum(np.abs(x))
    print(tag, "sum err", abs(got[0] - math.fsum(x)), "sum_abs err", abs(got[1] - sabs), "bound", 1e-12 * sabs)
    assert got[2] == x.min() and got[3] == x.max() and got[4] == np.abs(x).max(), tag
    assert abs(got[0] - math.fsum(x)) <= 1e-12 * sabs, tag
    assert abs(got[1] - sabs) <= 1e-12 * sabs, tag


def _reduce(env, form, arrays, level, masks):
    torch, capi, po, ws = env
    res = torch.full((len(arrays), 5), 7.0, dtype=torch.float64, device="cuda")
    fn = capi.p1_reduce_cells if form == "vertex" else capi.p2_edge_reduce_cells
    fn([a.data_ptr() for a in arrays], level, masks, res.data_ptr(), ws.data_ptr())
    return res.cpu().numpy()


def test_vectorised_slots_are_the_oracles(env):
    _, _, po, _ = env
    for level in range(0, 6):
        assert np.array_equal(_slots(po, level), po.slot_of_points(level)), level


@pytest.mark.parametrize("level", [0, 1, 2, 5, 6, 8])
def test_vertex_form_matches_numpy(env, level):
    """levels 0, 1: no interior; 2: one interior point; 5: rows shorter than a wave, and the smallest level with more than one
    workgroup per cell (46); 6: rows longer than 64 lanes; 8: 1024 workgroups per cell, several tiles each"""
    torch, capi, po, _ = env
    assert po.cell_size(level) == capi.cell_size(level)
    for k, mask in enumerate(MASKS):
        sel = _vertex_selected(po, level, mask)
        assert sel.size == po.cell_size(level)
        h = _field(1000 * level + k, sel)
        d = _dev(torch, h)
        got = _reduce(env, "vertex", [d], level, [mask])[0]
        _check(got, h[sel], ("vertex", level, hex(mask)))
        assert np.array_equal(d.cpu().numpy(), h), "the input array was written"
    assert _vertex_selected(po, level, 0x7FFF).all()


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5, 6])
def test_edge_form_matches_numpy(env, level):
    """level 5 (162 tiles) is the smallest level with more than one workgroup per cell, level 6 (1,244 tiles on 1024 workgroups)
    the smallest at which a workgroup strides"""
    torch, capi, po, _ = env
    n = po.edge_array_size(level)
    assert n == capi.p2_edge_array_size(level)
    for k, mask in enumerate(MASKS):
        sel = _edge_selected(po, level, mask)
        assert sel.size == n
        h = _field(2000 * level + k, sel)
        d = _dev(torch, h)
        got = _reduce(env, "edge", [d], level, [mask])[0]
        _check(got, h[sel], ("edge", level, hex(mask)))
        assert np.array_equal(d.cpu().numpy(), h), "the input array was written"
    assert _edge_selected(po, level, 0x7FFF).all()


@pytest.mark.parametrize("level", [3, 6])
def test_spike_known_answer(env, level):
    """FindMaxMinMagTest.cpp:47-49, 120-130 on one tetrahedron: a field of zeros with one spike of +100 or -200 at a macro-vertex,
    on a macro-edge, on a macro-face, inside the cell and in the last array entry -> max 100, min -200, magnitude 200"""
    torch, capi, po, _ = env
    n, N = po.cell_size(level), po.width(level)
    m, q = (N - 1) // 2, (N - 1) // 4
    vertices = [(0, 0, 0), (N - 1, 0, 0), (0, N - 1, 0), (0, 0, N - 1)]
    edges = [(m, 0, 0), (0, m, 0), (m, m, 0), (0, 0, m), (m, 0, m), (0, m, m)]
    faces = [(q, q, 0), (q, 0, q), (0, q, q), (q, q, N - 1 - 2 * q)]
    inner = np.flatnonzero(po.slot_of_points(level) == 14)
    spots = [po.cell_index(level, *p) for p in vertices + edges + faces] + [int(inner[0]), int(inner[-1]), n - 1]
    slots = po.slot_of_points(level)
    assert sorted(slots[spots[:14]]) == list(range(14)) and len(set(spots)) >= 16
    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    for i in spots:
        for spike in (100.0, -200.0):
            d[i] = spike
            got = [float(v) for v in _reduce(env, "vertex", [d], level, [0x7FFF])[0]]
            assert got == [spike, abs(spike), min(spike, 0.0), max(spike, 0.0), abs(spike)], (i, spike)
            d[i] = 0.0
    # the reference's three answers from one field: +100 at the first spot, -200 at the last
    d[spots[0]], d[spots[-1]] = 100.0, -200.0
    got = [float(v) for v in _reduce(env, "vertex", [d], level, [0x7FFF])[0]]
    assert (got[3], got[2], got[4]) == (100.0, -200.0, 200.0) and got[:2] == [-100.0, 300.0]


@pytest.mark.parametrize("form", ["vertex", "edge"])
def test_empty_mask_gives_the_starting_values(env, form):
    torch, capi, po, _ = env
    for level in (0, 3, 6):
        n = po.cell_size(level) if form == "vertex" else po.edge_array_size(level)
        d = _dev(torch, np.full(n, SENTINEL))
        for mask in (0, 0x8000):
            assert [float(v) for v in _reduce(env, form, [d], level, [mask])[0]] == EMPTY


def _batch_masks(ncells):
    """a different mask per cell; cell 1 (cell 0 of a single-cell batch excepted) has mask 0"""
    base = [0x4000 | 0x2A5, 0, 0x3FFF, 1 << 14, 0x7FFF]
    more = [int(m) for m in np.random.default_rng(ncells).permutation(np.arange(1, 0x7FFF)) if int(m) not in base]
    return (base + more)[:ncells]


@pytest.mark.parametrize("form,level", [("vertex", 3), ("vertex", 5), ("vertex", 6), ("edge", 2), ("edge", 5)])
@pytest.mark.parametrize("ncells", [1, 3, MAX_BATCH])
def test_batch_is_each_cell_alone_bit_for_bit(env, form, level, ncells):
    """different arrays and masks per cell, one mask 0: a cell's five numbers are bit-equal to that cell reduced alone (they do
    not depend on ncells or on the cell's position), equal numpy's, and a second identical call returns the same bits"""
    torch, capi, po, _ = env
    selected = _vertex_selected if form == "vertex" else _edge_selected
    masks = _batch_masks(ncells)
    host = [_field(31 * ncells + c, selected(po, level, m)) for c, m in enumerate(masks)]
    dev = [_dev(torch, h) for h in host]
    got = _reduce(env, form, dev, level, masks)
    again = _reduce(env, form, dev, level, masks)
    assert got.tobytes() == again.tobytes()
    for c in sorted({0, 1, ncells // 2, ncells - 1} & set(range(ncells))):
        alone = _reduce(env, form, [dev[c]], level, [masks[c]])[0]
        assert alone.tobytes() == got[c].tobytes(), c
        # and at another position of another batch
        if ncells > 1:
            moved = _reduce(env, form, [dev[0], dev[c]], level, [masks[0], masks[c]])[1]
            assert moved.tobytes() == got[c].tobytes(), c
    for c in range(ncells):
        _check(got[c], host[c][selected(po, level, masks[c])], (form, level, ncells, c))
    if ncells > 1:
        assert [float(v) for v in got[1]] == EMPTY
