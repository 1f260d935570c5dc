"""GPU tests of hyteg_hip_p1_cg_update_cells (hyteg_amd/csrc/p1_cg_update.hip) through the C-ABI: x += alpha p and r -= alpha ap on the
points of one mask, the sum of r * r over the points of another, in one pass -- against numpy on the same data, entry by entry."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INNER, ALL, SHELL = 0x4000, 0x7FFF, 0x3FFF
TILE = 1024           # entries per workgroup (kTile of p1_cg_update.hip)
TICKET_MAX = 128      # up to this many workgroups: one launch, the last workgroup reduces (kTicketBlocks)

# name: (level, update masks, dot masks, alpha)
CASES = {
    "level 2, the single inner point": (2, [INNER], [INNER], 0.75),
    "level 3, every point": (3, [ALL], [ALL], -1.25),
    # per-cell masks that differ; cell 1 is not touched; cell 2 updates its shell only and counts inner points it does not update
    "level 5, three cells": (5, [INNER | 0x2A5, 0, SHELL], [INNER | 0x0A5, 0, INNER | 0x3C0], -0.3125),
    "level 7, two cells": (7, [INNER | 0x0C0, INNER | 0x300], [INNER | 0x040, INNER], 0.4375),
}


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


def _tiles_per_cell(level, capacity=TILE):
    N = (1 << level) + 1
    return sum(((N - z) * (N - z + 1) // 2 + capacity - 1) // capacity for z in range(N))


def _workgroups(level, update_masks, dot_masks):
    return _tiles_per_cell(level) * sum(1 for u, d in zip(update_masks, dot_masks) if u | d)


def _call(torch, capi, arrays, alpha, level, update_masks, dot_masks):
    """fresh device copies of (x, r, p, ap), one call; returns the four arrays and the result as numpy"""
    dev = [_dev(torch, a) for a in arrays]
    nc = arrays[0].shape[0]
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    res = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
    capi.p1_cg_update_cells(*[[d[c].data_ptr() for c in range(nc)] for d in dev], alpha, level, update_masks, dot_masks, res.data_ptr(),
                            ws.data_ptr())
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dev], float(res.cpu()[0])


def test_the_cases_cover_both_reduction_tails():
    """as test_gpu_cg_device.py does for the dot product: one case on either side of the ticket threshold, several tiles per cell"""
    assert _tiles_per_cell(5) > 1
    assert 1 < _workgroups(*CASES["level 5, three cells"][:3]) <= TICKET_MAX < _workgroups(*CASES["level 7, two cells"][:3])
    assert _workgroups(*CASES["level 7, two cells"][:3]) <= 1024  # every workgroup owns one tile: no grid stride yet


@pytest.mark.parametrize("case", list(CASES))
def test_cg_update_cells_against_numpy(env, case):
    torch, capi, host, po = env
    import hostutil as hu

    level, update_masks, dot_masks, alpha = CASES[case]
    nc, n = len(update_masks), po.cell_size(level)
    rng = np.random.default_rng(level)
    x, r, p, ap = (rng.standard_normal((nc, n)) for _ in range(4))
    (gx, gr, gp, gap), result = _call(torch, capi, (x, r, p, ap), alpha, level, update_masks, dot_masks)
    assert np.array_equal(gp, p) and np.array_equal(gap, ap)  # never written
    squares = []
    for c in range(nc):
        upd, dot = hu.point_mask(level, update_masks[c]), hu.point_mask(level, dot_masks[c])
        if level == 2:
            assert upd.sum() == 1
        # one fused multiply-add or a multiplication and an addition, plus numpy's own rounding of the comparison value
        for got, old, step in ((gx[c], x[c], alpha * p[c]), (gr[c], r[c], -alpha * ap[c])):
            assert (np.abs(got[upd] - (old[upd] + step[upd])) <= 2.0 ** -51 * (np.abs(old[upd]) + np.abs(step[upd]))).all()
            assert np.array_equal(got[~upd], old[~upd])  # every other entry keeps its bits
            if upd.any():
                assert not np.array_equal(got[upd], old[upd])
        squares += [float(v) * float(v) for v in gr[c][dot]]
    want = math.fsum(squares)
    assert want > 0.0 and result != 1e300
    assert abs(result - want) <= 1e-12 * want, (result, want)
    # fixed summation order: a second call on fresh copies of the same inputs gives the same bits everywhere
    again, result2 = _call(torch, capi, (x, r, p, ap), alpha, level, update_masks, dot_masks)
    assert result2 == result
    for a, b in zip(again, (gx, gr, gp, gap)):
        assert np.array_equal(a, b)


def test_cg_update_cells_with_nothing_selected_gives_zero(env):
    torch, capi, host, po = env
    n = po.cell_size(3)
    arrays = tuple(np.random.default_rng(k).standard_normal((2, n)) for k in range(4))
    got, result = _call(torch, capi, arrays, 0.5, 3, [0, 0], [0, 0])
    assert result == 0.0
    for a, b in zip(got, arrays):
        assert np.array_equal(a, b)


def test_cg_update_cells_rejects_bad_arguments_before_any_gpu_work(env):
    torch, capi, host, po = env
    level = 3
    n = po.cell_size(level)
    host_arrays = [np.random.default_rng(10 + k).standard_normal(n) for k in range(4)]
    x, r, p, ap = (_dev(torch, a) for a in host_arrays)
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    res = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
    X, R, P, AP, W, S = [x.data_ptr()], [r.data_ptr()], [p.data_ptr()], [ap.data_ptr()], ws.data_ptr(), res.data_ptr()
    many = capi.HYTEG_HIP_MAX_BATCH + 1
    bad = {
        "level below range": (X, R, P, AP, 0.5, -1, [ALL], [ALL], S, W),
        "level above range": (X, R, P, AP, 0.5, 12, [ALL], [ALL], S, W),
        "no cells": ([], [], [], [], 0.5, level, [], [], S, W),
        "too many cells": (X * many, R * many, P * many, AP * many, 0.5, level, [ALL] * many, [ALL] * many, S, W),
        "null x": (None, R, P, AP, 0.5, level, [ALL], [ALL], S, W),
        "null ap": (X, R, P, None, 0.5, level, [ALL], [ALL], S, W),
        "null update masks": (X, R, P, AP, 0.5, level, None, [ALL], S, W),
        "null dot masks": (X, R, P, AP, 0.5, level, [ALL], None, S, W),
        "null result": (X, R, P, AP, 0.5, level, [ALL], [ALL], None, W),
        "null workspace": (X, R, P, AP, 0.5, level, [ALL], [ALL], S, None),
        "null array of a cell": (X, [0], P, AP, 0.5, level, [ALL], [ALL], S, W),
        "x is r": (X, X, P, AP, 0.5, level, [ALL], [ALL], S, W),
        "x is p": (X, R, X, AP, 0.5, level, [ALL], [ALL], S, W),
        "x is ap": (X, R, P, X, 0.5, level, [ALL], [ALL], S, W),
        "r is p": (X, R, R, AP, 0.5, level, [ALL], [ALL], S, W),
        "r is ap": (X, R, P, R, 0.5, level, [ALL], [ALL], S, W),
    }
    for name, args in bad.items():
        with pytest.raises(capi.HytegHipError):
            capi.p1_cg_update_cells(*args)
            pytest.fail(name)
    torch.cuda.synchronize()
    for d, h in zip((x, r, p, ap), host_arrays):
        assert np.array_equal(d.cpu().numpy(), h)
    assert float(res.cpu()[0]) == 1e300
    # p may be ap: only x and r are written
    capi.p1_cg_update_cells(X, R, P, P, 0.5, level, [ALL], [ALL], S, W)
    torch.cuda.synchronize()
    assert float(res.cpu()[0]) != 1e300
