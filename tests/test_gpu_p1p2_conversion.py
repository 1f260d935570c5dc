"""P1toP2Conversion / P2toP1Conversion on the GPU through the C-ABI (hyteg_amd/csrc/kernels_p1p2_conversion.hpp): the
conversion is a permutation, so every comparison is np.array_equal against the numpy map of tests/conversionutil.py (pinned to
the oracle's indexing in tests/test_p1p2_conversion_map.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

# P2 levels: 0 has an empty XYZ block, 1 the first XYZ entry, 6 has fine rows of 129 entries, one more than a wave's run of 128
LEVELS = [0, 1, 2, 3, 6]
MASKS = [0x7FFF, 1 << 14, 0x03C0 | (1 << 14), 0x003F, 0]


@pytest.fixture(scope="module")
def env():
    import torch

    import conversionutil as cu
    from hyteg_amd import capi

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi, cu


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _random_arrays(cu, level, seed):
    nv, ne, nf = cu.sizes(level)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nf), rng.standard_normal(nv), rng.standard_normal(ne)


@pytest.mark.parametrize("level", LEVELS)
def test_p1_to_p2_is_the_permutation_on_the_selected_dofs(env, level):
    torch, capi, cu = env
    p1, v0, e0 = _random_arrays(cu, level, level)
    p1d = _dev(torch, p1)
    for mask in MASKS:
        vd, ed = _dev(torch, v0), _dev(torch, e0)
        capi.p1_to_p2_cell(vd.data_ptr(), ed.data_ptr(), p1d.data_ptr(), level, mask)
        torch.cuda.synchronize()
        wv, we = cu.p1_to_p2_expected(p1, v0, e0, level, mask)
        assert np.array_equal(vd.cpu().numpy(), wv) and np.array_equal(ed.cpu().numpy(), we), hex(mask)
        assert np.array_equal(p1d.cpu().numpy(), p1)  # the source is only read
    # the masks above are not vacuous: the full one selects every DoF, the interior one some from P2 level 1 on (the XYZ DoF)
    assert cu.selected(level, 0x7FFF).all() and cu.selected(level, 1 << 14).any() == (level >= 1)


@pytest.mark.parametrize("level", LEVELS)
def test_p2_to_p1_is_the_permutation_on_the_selected_dofs(env, level):
    torch, capi, cu = env
    p0, v, e = _random_arrays(cu, level, 20 + level)
    vd, ed = _dev(torch, v), _dev(torch, e)
    for mask in MASKS:
        pd = _dev(torch, p0)
        capi.p2_to_p1_cell(pd.data_ptr(), vd.data_ptr(), ed.data_ptr(), level, mask)
        torch.cuda.synchronize()
        assert np.array_equal(pd.cpu().numpy(), cu.p2_to_p1_expected(p0, v, e, level, mask)), hex(mask)
        assert np.array_equal(vd.cpu().numpy(), v) and np.array_equal(ed.cpu().numpy(), e)


@pytest.mark.parametrize("level", LEVELS)
def test_round_trip_is_the_identity(env, level):
    torch, capi, cu = env
    p1, v0, e0 = _random_arrays(cu, level, 40 + level)
    p1d, vd, ed = _dev(torch, p1), _dev(torch, v0), _dev(torch, e0)
    back = torch.zeros_like(p1d)
    capi.p1_to_p2_cell(vd.data_ptr(), ed.data_ptr(), p1d.data_ptr(), level)
    capi.p2_to_p1_cell(back.data_ptr(), vd.data_ptr(), ed.data_ptr(), level)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), p1)
    # and every P2 entry was written: nothing of the random start is left
    both = np.concatenate([vd.cpu().numpy(), ed.cpu().numpy()])
    assert np.array_equal(np.sort(both), np.sort(p1))


@pytest.mark.parametrize("level", [1, 3, 6])
def test_batch_of_three_cells_equals_the_per_cell_calls(env, level):
    torch, capi, cu = env
    masks = [0x7FFF, 0, 0x03C0 | (1 << 14)]
    data = [_random_arrays(cu, level, 60 + 3 * level + c) for c in range(3)]
    for to_p2 in (True, False):
        batch = [[_dev(torch, a) for a in cell] for cell in data]  # per cell: p1, vertex, edge
        single = [[_dev(torch, a) for a in cell] for cell in data]
        p, v, e = ([cell[k].data_ptr() for cell in batch] for k in range(3))
        if to_p2:
            capi.p1_to_p2_cells(v, e, p, level, masks)
        else:
            capi.p2_to_p1_cells(p, v, e, level, masks)
        for cell, mask in zip(single, masks):
            if to_p2:
                capi.p1_to_p2_cell(cell[1].data_ptr(), cell[2].data_ptr(), cell[0].data_ptr(), level, mask)
            else:
                capi.p2_to_p1_cell(cell[0].data_ptr(), cell[1].data_ptr(), cell[2].data_ptr(), level, mask)
        torch.cuda.synchronize()
        for c in range(3):
            for k in range(3):
                assert np.array_equal(batch[c][k].cpu().numpy(), single[c][k].cpu().numpy())
        # the cell with mask 0 is untouched, the others are not
        for k in range(3):
            assert np.array_equal(batch[1][k].cpu().numpy(), data[1][k])
        changed = 1 if to_p2 else 0
        assert not np.array_equal(batch[0][changed].cpu().numpy(), data[0][changed])


def test_level_7_against_a_device_index(env):
    """fine rows of 257 entries (three runs of a wave): compared on the device with a torch index built from the numpy map"""
    torch, capi, cu = env
    level = 7
    nv, ne, nf = cu.sizes(level)
    _, _, target = cu.p1_to_p2_map(level)
    t = torch.from_numpy(target.copy()).cuda()  # the cached map is read-only
    gen = torch.Generator(device="cuda").manual_seed(7)
    p1 = torch.randn(nf, dtype=torch.float64, device="cuda", generator=gen)
    v, e = torch.zeros(nv, dtype=torch.float64, device="cuda"), torch.zeros(ne, dtype=torch.float64, device="cuda")
    capi.p1_to_p2_cell(v.data_ptr(), e.data_ptr(), p1.data_ptr(), level)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([v, e])[t], p1)
    back = torch.zeros_like(p1)
    capi.p2_to_p1_cell(back.data_ptr(), v.data_ptr(), e.data_ptr(), level)
    torch.cuda.synchronize()
    assert torch.equal(back, p1)
    # interior only: the boundary points keep their value
    inner = torch.from_numpy(cu.selected(level, 1 << 14).copy()).cuda()
    part = torch.full_like(p1, -1.0)
    capi.p2_to_p1_cell(part.data_ptr(), v.data_ptr(), e.data_ptr(), level, 1 << 14)
    torch.cuda.synchronize()
    assert torch.equal(part, torch.where(inner, p1, torch.full_like(p1, -1.0)))
